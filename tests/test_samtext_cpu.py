"""Pass C of phase 2 without a GPU.
 * bmh_sam_text_batch against the Python restatement of the reference's lines (tests/samtext_ref.py), byte for byte, on the constructed
   slices of tests/samtextgen.py -- whose shapes are counted and asserted here -- and on phase2gen's vectors through the host's pass A.
 * every refusal leaves sentinel-filled outputs untouched.
 * host/samtext_core.h as a stand-alone program (tests/samtext_core_main.c), built plainly and with -fsanitize=address,undefined: counted
   size == written size == the host call's for every read, and a slice one byte short is refused without a byte written past it.
 * where oracle/_ref is built: the restatement's line emitter against the reference's own mem_aln2sam, live."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
import samtext_ref as ref
import samtextgen as sg
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "samtext_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def host_text(pkg, sl, idx=None, **kw):
    text, off = pkg.sam_text_batch(sl["opt"], idx if idx is not None else sg.refidx(), sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"],
                                   sl["cig"], sl["md"], sl["rg_id"], **kw)
    assert off[0] == 0 and len(text) == off[-1] and b"\0" not in text
    return [text[int(off[i]):int(off[i + 1])] for i in range(len(sl["seqs"]))]


def same(got, want):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (len(bad), bad[:5], got[bad[0]][:400], want[bad[0]][:400])


@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
@pytest.mark.parametrize("units", [1, 65, 257])
def test_host_call_is_the_restatement(pkg, mode, units):
    sl = sg.make(mode, units, seed=units)
    same(host_text(pkg, sl), sg.expected(sl))


@pytest.mark.parametrize("mode,flag", [("se", sg.NO_MULTI), ("pe-all", sg.NO_MULTI), ("pe", sg.NOPAIRING)])
def test_host_call_under_other_flags(pkg, mode, flag):
    sl = sg.make(mode, 130, seed=5, flag=flag)
    exp = sg.expected(sl)
    same(host_text(pkg, sl), exp)
    s = sg.shapes(sl, exp)
    if flag == sg.NO_MULTI:  # 0x10000 is shown as 0x100, with SEQ and QUAL, and never as 0x800
        assert s["no_multi"] >= 20 and s["supplementary"] == 0
    else:  # no proper-pair test of the top hits: only a paired decision's lines carry 0x2
        assert s["top_proper"] == 0 and s["top_improper"] >= 20


def test_the_slices_hold_what_they_claim(pkg):
    se = sg.make("se-all", 257, seed=1)
    s = sg.shapes(se, sg.expected(se))
    assert s["lead_trail_del"] >= 50 and s["secondary"] >= 50 and s["supplementary"] >= 100 and s["hard"] >= 100
    assert s["sa1"] >= 30 and s["sa3"] >= 30 and s["unmapped"] >= 16 and s["many"] >= 8 and s["l_seq_1"] >= 8
    assert s["no_qual"] >= 8 and 0 < s["comment"] < s["lines"] and s["rg"] == s["lines"] and s["capped"] >= 20
    assert {1, 250} <= s["name_lens"] and s["pos_digits"] == set(range(1, 11)) and s["rev_past_2_32"] >= 100
    assert sg.make("se", 65, seed=2)["rg_id"] == b"" and sg.shapes(se, sg.expected(sg.make("se", 65, seed=2)))["rg"] == 0
    pe = sg.make("pe-all", 257, seed=1)
    p = sg.shapes(pe, sg.expected(pe))
    assert p["mate_unmapped"] >= 20 and p["mate_other"] >= 20 and p["tlen_pos"] >= 50 and p["tlen_neg"] >= 50 and p["tlen_zero"] >= 5
    assert p["top_proper"] >= 20 and p["top_improper"] >= 20 and p["capped"] >= 5 and p["secondary"] >= 10
    assert p["neg_tlen_digits"] == set(range(1, 11)), p["neg_tlen_digits"]
    lens = {len(x[2]) for x in se["seqs"]}
    assert 1 in lens and min(lens - {1}) >= 30 and max(lens) <= 300


def _fabricate(pkg, reads, host):
    """records and pools for the wanted regions of decided vectors: M runs with one insertion or deletion that makes up the difference"""
    res, cig, md = [], [], bytearray()
    for rd, v, ks in zip(reads, host["regs"], host["want"]):
        for k in ks:
            a = v[int(k)]
            ql, tl = int(a["qe"]) - int(a["qb"]), int(a["re"]) - int(a["rb"])
            m = min(ql, tl)
            words = [m << 4] if ql == tl else [(m // 2) << 4, abs(ql - tl) << 4 | (1 if ql > tl else 2), (m - m // 2) << 4]
            x = np.zeros((), dtype=pkg.WANTED_RES)
            x["rb"], x["re"], x["qb"], x["qe"], x["score"], x["n_cigar"], x["NM"] = a["rb"], a["re"], a["qb"], a["qe"], a["score"], len(words), abs(ql - tl)
            s = b"%d" % m
            x["cigar_off"], x["md_off"], x["md_len"] = len(cig), len(md), len(s)
            cig += words
            md += s + b"\0"
            res.append(x)
    return (np.array(res, dtype=pkg.WANTED_RES).reshape(-1), np.array(cig + [0], dtype=np.uint32), np.frombuffer(bytes(md) + b"\0", dtype=np.uint8).copy())


def phase2_slice(pkg, mode, units, seed=0):
    """phase2gen's vectors through the host's pass A, with fabricated alignments: real decisions, real coordinates"""
    import phase2gen as pg
    import wantgen as wg
    o, pes, id0, reads, vectors = pg.make(mode, units=units, seed=seed)
    host = pg.decide(o, pes, id0, vectors)
    res, cig, md = _fabricate(pkg, reads, host)
    pe = mode.startswith("pe")
    seqs = [(b"q%d" % (i // 2 if pe else i), None, np.asarray(r, dtype=np.uint8), bytes([40 + i % 30]) * len(r)) for i, r in enumerate(reads)]
    return dict(opt=o, pes=pes, seqs=seqs, vectors=host["regs"], dec=host, res=res, cig=cig, md=md, rg_id=b"",
                contigs=wg.CONTIGS, l_pac=wg.L_PAC, names=[b"seq%d" % i for i in range(len(wg.CONTIGS))])


@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
def test_host_call_on_decided_vectors(pkg, mode):
    sl = phase2_slice(pkg, mode, 60)
    exp = ref.slice_text(sl["opt"], sl["contigs"], sl["names"], sl["l_pac"], sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"], sl["cig"],
                         sl["md"], sl["rg_id"])
    same(host_text(pkg, sl, idx=pkg.make_refidx(sl["contigs"], sl["l_pac"])), exp)
    assert sum(len(t.split(b"\n")) - 1 for t in exp) > len(exp)  # (some read prints more than one line)


@pytest.mark.parametrize("mode", ["se-all", "pe"])
def test_refusals_leave_the_outputs_untouched(pkg, mode):
    sl = sg.make(mode, 20, seed=3)
    idx = sg.refidx()
    for what, bad in sg.refusals(sl):
        out = sg.sentinels(len(bad["seqs"]))
        with pytest.raises(pkg.BmhError) as e:
            host_text(pkg, bad, idx=idx, out=out)
        assert e.value.code == pkg.BMH_E_ARG, what
        assert out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all(), what
    lib = pkg.lib()
    t, off = C.c_void_p(0x5a5a5a5a), np.full(1, -77, dtype=np.int64)
    o = sl["opt"].reshape(1)
    tail = [None] * 10 + [b""]
    assert lib.bmh_sam_text_batch(o.ctypes.data, C.byref(idx), None, -1, *tail, C.byref(t), off.ctypes.data) == pkg.BMH_E_ARG
    assert lib.bmh_sam_text_batch(None, C.byref(idx), None, 0, *tail, C.byref(t), off.ctypes.data) == pkg.BMH_E_ARG
    assert lib.bmh_sam_text_batch(o.ctypes.data, None, None, 0, *tail, C.byref(t), off.ctypes.data) == pkg.BMH_E_ARG
    assert lib.bmh_sam_text_batch(o.ctypes.data, C.byref(idx), None, 0, *tail, None, off.ctypes.data) == pkg.BMH_E_ARG
    assert lib.bmh_sam_text_batch(o.ctypes.data, C.byref(idx), None, 0, *tail, C.byref(t), None) == pkg.BMH_E_ARG
    assert t.value == 0x5a5a5a5a and off[0] == -77


def test_no_read(pkg):
    sl = sg.make("se", 0)
    text, off = pkg.sam_text_batch(sl["opt"], sg.refidx(), None, [], [], sl["dec"], None, None, None, b"")
    assert text == b"" and off.tolist() == [0]


# ---------------------------------------------------------------- the core as a program of its own

def dump(pkg, sl, path):
    text, off = pkg.sam_text_batch(sl["opt"], sg.refidx(), sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"], sl["cig"], sl["md"], sl["rg_id"])
    n, pe = len(sl["seqs"]), int(bool(int(sl["opt"]["flag"]) & sg.PE))
    roff = np.concatenate([[0], np.cumsum([len(v) for v in sl["vectors"]])]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(sl["dec"]["n_want"])]).astype(np.int64)
    total, n_w = int(roff[-1]), int(first[-1])
    refspan = np.zeros(len(sg.CONTIGS), dtype=[("offset", "<i8"), ("len", "<i4"), ("rsv", "<i4")])
    refspan["offset"], refspan["len"] = [c[0] for c in sg.CONTIGS], [c[1] for c in sg.CONTIGS]
    noff = np.concatenate([[0], np.cumsum([len(x) for x in sg.NAMES])]).astype(np.uint64)
    poff, pool = sg.pack_reads(sl["seqs"])
    pes = sl["pes"] if sl["pes"] is not None else np.zeros(4, dtype=kswlib.PESTAT)
    regs = np.concatenate([v for v in sl["vectors"] if len(v)]) if total else np.zeros(0, dtype=kswlib.ALNREG)
    hd = np.array([n, pe, int(sl["opt"]["flag"]), sg.L_PAC, len(sg.CONTIGS), total, n_w, len(sl["cig"]), len(sl["md"]), int(noff[-1]), len(sl["rg_id"]),
                   len(pool)], dtype=np.int64)
    with open(path, "wb") as f:
        for a in (hd, refspan, noff, b"".join(sg.NAMES), np.ascontiguousarray(pes, dtype=kswlib.PESTAT), roff, first, sl["dec"]["n_want"].astype(np.int32),
                  sl["dec"]["want_k"][:total].astype(np.int32), sl["dec"]["reg_mapq"][:total].astype(np.int32), sl["dec"]["pd"], regs, sl["res"],
                  sl["cig"], sl["md"], sl["rg_id"], poff, pool, off, text):
            f.write(a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes())
    return n, sum(t.count(b"\n") for t in [text]), len(text)


@pytest.fixture(scope="module")
def dumps(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("samtext")
    out = []
    for mode, units, flag in (("se-all", 130, 0), ("pe-all", 130, 0), ("se", 40, sg.NO_MULTI)):
        path = d / f"{mode}_{flag}.bin"
        out.append((path, dump(pkg, sg.make(mode, units, seed=9, flag=flag), path)))
    return out


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-lm"], capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, dumps):
    for path, (n, lines, nbytes) in dumps:
        run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert run.returncode == 0, f"exit {run.returncode}\n{run.stderr[-4000:]}"
        assert run.stdout.split() == ["ok", str(n), str(lines), str(nbytes)]


def test_core_program_counts_what_it_writes(dumps, tmp_path):
    _, exe, cc = _build(tmp_path, "samtext_plain", [])
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    _run(exe, dumps)


def test_core_program_under_sanitizers(dumps, tmp_path):
    gcc, _, plain = _build(tmp_path, "samtext_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "samtext_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, dumps)


# ---------------------------------------------------------------- the restatement's emitter against the reference's own

class _RefAnn(C.Structure):  # bntann1_t, bntseq.h:39-45
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("name", C.c_char_p), ("anno", C.c_char_p)]


class _RefBns(C.Structure):  # bntseq_t, bntseq.h:53-61
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(_RefAnn)), ("n_holes", C.c_int32),
                ("ambs", C.c_void_p), ("fp_pac", C.c_void_p)]


class _RefAln(C.Structure):  # mem_aln_t, bwamem.h:72-81 (is_rev:1, mapq:8, NM:23 in one word)
    _fields_ = [("pos", C.c_int64), ("rid", C.c_int), ("flag", C.c_int), ("bits", C.c_uint32), ("n_cigar", C.c_int), ("cigar", C.c_void_p),
                ("score", C.c_int), ("sub", C.c_int)]


class _RefSeq(C.Structure):  # bseq1_t, bwa.h:19-22
    _fields_ = [("l_seq", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


class _KString(C.Structure):  # kstring_t, kstring.h:17-20
    _fields_ = [("l", C.c_size_t), ("m", C.c_size_t), ("s", C.c_void_p)]


@pytest.mark.ref
def test_restatement_emitter_against_the_reference(pkg):
    """mem_aln2sam itself, live, on the mem_aln_t lists the restatement forms from the constructed slices (every list, every line, with
    the mate it is printed with): the same bytes.  That pins samtext_ref.aln2sam, which the other tests compare the library with."""
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    rl = reflib.lib()
    rl.mem_aln2sam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    rl.mem_aln2sam.restype = None
    rg = (C.c_char * 256).in_dll(rl, "bwa_rg_id")
    anns = (_RefAnn * len(sg.CONTIGS))(*[_RefAnn(o, n, 0, 0, nm, b"") for (o, n), nm in zip(sg.CONTIGS, sg.NAMES)])
    bns = _RefBns(sg.L_PAC, len(sg.CONTIGS), 11, anns, 0, None, None)
    keep = []

    def c_aln(a):
        buf = np.zeros(len(a.cigar) + (len(a.md) + 4) // 4 + 1, dtype=np.uint32)  # the MD string lies behind the CIGAR words
        buf[:len(a.cigar)] = a.cigar
        buf[len(a.cigar):].view(np.uint8)[:len(a.md)] = np.frombuffer(a.md, dtype=np.uint8)
        keep.append(buf)
        assert 0 <= a.mapq < 256 and 0 <= a.NM < 1 << 23
        return _RefAln(a.pos, a.rid, a.flag, a.is_rev | a.mapq << 1 | a.NM << 9, len(a.cigar), buf.ctypes.data, a.score, a.sub)

    calls = []
    orig = ref.aln2sam

    def spy(names, rg_id, s, lst, which, m):
        out = orig(names, rg_id, s, lst, which, m)
        calls.append((rg_id, s, [x.copy() for x in lst], which, m.copy() if m is not None else None, out))
        return out
    ref.aln2sam = spy
    try:
        for mode, flag in (("se-all", 0), ("pe-all", 0), ("se", sg.NO_MULTI), ("pe", 0)):
            sl = sg.make(mode, 130, seed=4 + (mode == "pe"), flag=flag)
            sg.expected(sl)
    finally:
        ref.aln2sam = orig
    assert len(calls) > 1500
    try:
        for rg_id, (name, com, seq, qual), lst, which, m, out in calls:
            rg.value = rg_id
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            s = _RefSeq(len(seq), name, com, seq.ctypes.data, qual, None)
            arr = (_RefAln * len(lst))(*[c_aln(x) for x in lst])
            mate = c_aln(m) if m is not None else None
            ks = _KString(0, 0, None)
            rl.mem_aln2sam(C.byref(bns), C.byref(ks), C.byref(s), len(lst), arr, which, C.byref(mate) if mate is not None else None)
            got = C.string_at(ks.s, ks.l)
            reflib._libc.free(ks.s)
            assert got == out, (got[:300], out[:300])
            keep.clear()
    finally:
        rg.value = b""
