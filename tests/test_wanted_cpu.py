"""Pass B of phase 2 without a GPU.
 * host/regplan_core.h as a stand-alone program (tests/regplan_core_main.c), built plainly and with -fsanitize=address,undefined and run
   as a program of its own, against the Python restatement of the reference's lines (tests/regplan.py): bands, tries and tasks, the
   emitted record and task bytes, bns_pos2rid, the test of bwa_fix_xref2 and its walk to the cut points.  The undefined-behaviour
   build also shows that no arithmetic touches truesc == INT32_MIN.
 * the interface: the new calls are declared and exported, bmh_version() is still 310, bad arguments are refused before a device is
   touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import regplan as rp
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "regplan_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CONTIGS = [(0, 3000), (3000, 1001), (4001, 507)]
L_PAC = 4508


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _band_cases():
    rng = np.random.default_rng(20)
    cases = []

    def add(ql, tl, truesc, reg_w, a, o_del, e_del, o_ins, e_ins, w):
        cases.append((int(ql), int(tl), int(truesc), int(reg_w), int(a), int(a), int(o_del), int(e_del), int(o_ins), int(e_ins), int(w)))
    for _ in range(6000):  # random lengths, scores and scoring
        ql = int(rng.integers(1, 400)) if rng.random() < 0.8 else int(rng.integers(1, 65536))
        tl = max(1, ql + int(rng.integers(-40, 41))) if rng.random() < 0.7 else int(rng.integers(1, 65536))
        tl = min(tl, 65535)
        a = int(rng.integers(1, 6))
        truesc = min(ql, tl) * a - int(rng.integers(0, 200)) if rng.random() < 0.8 else int(rng.integers(-100000, 400000))
        add(ql, tl, truesc, rng.integers(0, 300), a, rng.integers(0, 12), rng.choice([1, 2, 3, 7]), rng.integers(0, 12), rng.choice([1, 2, 3, 7]),
            rng.choice([0, 5, 100, 1000]))
    for e in (1, 2, 3, 7):  # ql == tl on both sides of l*a - score < (q + r - a) << 1, for every e; also a > q + r (a negative right side)
        for a, q in ((1, 6), (2, 4), (5, 1), (9, 0)):
            for ln in (1, 31, 150, 65535):
                lim = (q + e - a) * 2
                for d in (lim - 2, lim - 1, lim, lim + 1, lim + 7):
                    add(ln, ln, ln * a - d, 100, a, q, e, q, e, 100)
                    add(ln, ln, ln * a - d, 3, a, q + 3, e, q, (e % 7) + 1, 5)
    for ql, tl in ((1, 1), (150, 150), (150, 161), (12000, 12044), (65535, 65535), (65535, 1)):  # the single try of bwa_fix_xref2
        for reg_w in (0, 1, 5, 100, 70000):
            add(ql, tl, rp.INT32_MIN, reg_w, 1, 6, 1, 6, 1, 100)
    for w2_cap in (1, 2, 3, 40, 5000):  # a band that saturates: the tries share a task
        add(150, 150, 20, w2_cap, 1, 6, 1, 6, 1, 0)
        add(150, 152, -50, w2_cap, 1, 6, 1, 6, 1, 0)
    return cases


def _expected_band(c):
    ql, tl, truesc, reg_w, a, mat0, o_del, e_del, o_ins, e_ins, w = c
    o = {"a": a, "mat0": mat0, "o_del": o_del, "e_del": e_del, "o_ins": o_ins, "e_ins": e_ins, "w": w}
    w2, band, slot, n_tasks, cap = rp.plan(o, ql, tl, truesc, reg_w)
    req, tasks = rp.emit_hex(band, slot, n_tasks, cap, 1000, 77, 5000, ql, tl, truesc, 10, 240)
    return f"B {w2} {band[0]} {band[1]} {band[2]} {slot[0]} {slot[1]} {slot[2]} {n_tasks} {cap} {req} {tasks}".rstrip()


def _random_cigar(rng, rb, re, qb):
    """a CIGAR over the window [rb, re): M / I / D runs"""
    words, x = [], rb
    while x < re:
        op = int(rng.choice([0, 0, 0, 1, 2]))
        ln = int(rng.integers(1, 40))
        if op != 1:
            ln = min(ln, re - x)
            x += ln
        words.append(ln << 4 | op)
    return words


def _cases():
    rng = np.random.default_rng(21)
    lines, want = [], []
    bc = _band_cases()
    assert len(bc) >= 5000
    for c in bc:
        lines.append("B " + " ".join(map(str, c)))
        want.append(_expected_band(c))
    tables = [(CONTIGS, L_PAC), ([(0, 1)], 1), ([(0, 5), (5, 1), (6, 1), (7, 40)], 47), ([(i * 10, 10) for i in range(33)], 330)]
    for contigs, l_pac in tables:
        lines.append(f"R {len(contigs)} {l_pac} " + " ".join(f"{o} {n}" for o, n in contigs))
        ps = {0, l_pac - 1, l_pac, l_pac + 5}
        for off, ln in contigs:  # the first and the last base of every sequence, and their neighbours
            ps |= {off, off + ln - 1, max(off - 1, 0), min(off + 1, l_pac - 1)}
        ps |= {int(x) for x in rng.integers(0, l_pac, 50)}
        for pos in sorted(ps):
            lines.append(f"P {pos}")
            want.append(f"P {rp.pos2rid(contigs, l_pac, pos)}")
        for _ in range(400):
            strand = int(rng.integers(0, 2))
            b = int(rng.integers(0, l_pac))
            e = min(b + int(rng.integers(1, 200)), l_pac)
            rb, re = (b, e) if not strand else (2 * l_pac - e, 2 * l_pac - b)
            if rng.random() < 0.05:  # across the strands
                rb, re = l_pac - int(rng.integers(1, 20)), l_pac + int(rng.integers(1, 20))
            v, cb, ce = rp.xref_test(contigs, l_pac, rb, re)
            lines.append(f"X {rb} {re}")
            want.append(f"X {v} {cb} {ce}")
            if v == 1:
                qb = int(rng.integers(0, 30))
                cig = _random_cigar(rng, rb, re, qb)
                qe = qb + sum(w >> 4 for w in cig if (w & 0xf) != 2)
                lines.append(f"C {qb} {qe} {rb} {re} {cb} {ce} {len(cig)} " + " ".join(map(str, cig)))
                want.append("C %d %d %d %d %d" % rp.xref_cut(cig, cb, ce, qb, qe, rb, re))
    # the cut inside a deletion on either end, and a cut that leaves nothing
    for cig, cb, ce in (([40 << 4, 10 << 4 | 2, 50 << 4], 45, 100), ([40 << 4, 10 << 4 | 2, 50 << 4], 0, 44), ([5 << 4 | 1, 30 << 4 | 2, 60 << 4], 0, 25),
                        ([50 << 4], 50, 50), ([10 << 4, 5 << 4 | 2], 12, 15)):
        qe = 7 + sum(w >> 4 for w in cig if (w & 0xf) != 2)
        re = sum(w >> 4 for w in cig if (w & 0xf) != 1)
        lines.append(f"C 7 {qe} 0 {re} {cb} {ce} {len(cig)} " + " ".join(map(str, cig)))
        want.append("C %d %d %d %d %d" % rp.xref_cut(cig, cb, ce, 7, qe, 0, re))
    return lines, want


@pytest.fixture(scope="module")
def program_input(tmp_path_factory):
    lines, want = _cases()
    path = tmp_path_factory.mktemp("regplan") / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return path, want


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-lm"], capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stderr[-4000:]}"
    return [l.rstrip() for l in run.stdout.splitlines()]


def _compare(got, want):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (len(bad), bad[:5], got[bad[0]][:300], want[bad[0]][:300])


def test_cases_cover_what_they_claim():
    _, want = _cases()
    b = [l.split() for l in want if l.startswith("B ")]
    nogap = sum(l[2] == "-1" for l in b)
    single = sum(l[2] != "-1" and l[3] == "-1" for l in b)
    shared = sum(l[8] in ("1", "2") and l[4] != "-1" for l in b)
    three = sum(l[8] == "3" for l in b)
    assert min(nogap, single, shared, three) >= 16, (nogap, single, shared, three)
    c = [l.split() for l in want if l.startswith("C ")]
    assert sum(l[1] == "-2" for l in c) >= 1 and sum(l[1] == "0" for l in c) > 100
    assert {l.split()[1] for l in want if l.startswith("X ")} == {"-1", "0", "1"}


def test_core_program_prints_the_restatements_results(program_input, tmp_path):
    path, want = program_input
    _, exe, cc = _build(tmp_path, "regplan_plain", [])
    assert cc.returncode == 0, cc.stderr
    assert "warning" not in cc.stderr, cc.stderr
    _compare(_run(exe, path), want)


def test_core_program_under_sanitizers(program_input, tmp_path):
    path, want = program_input
    gcc, _, plain = _build(tmp_path, "regplan_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "regplan_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _compare(_run(exe, path), want)


# ---------------------------------------------------------------- the generator against the reference

def _pos_of(rb, re, words, l_pac, contigs):
    """mem_reg2aln's position (bwamem.c:1203-1212, :1231-1232): the leftmost base on the forward strand, past a leading deletion"""
    p = rb if rb < l_pac else re - 1
    is_rev = p >= l_pac
    if is_rev:
        p = (l_pac << 1) - 1 - p
    if len(words) and int(words[0]) & 0xf == 2:
        p += int(words[0]) >> 4
    return p - contigs[rp.pos2rid(contigs, l_pac, p)][0], int(is_rev)


@pytest.mark.ref
def test_generator_against_the_reference(tmp_path):
    """wantgen's constructed regions through the reference's own mem_reg2aln (bwa_fix_xref2 included): the restatement's fixed coordinates
    plus the oracle's alignment must give the reference's pos, CIGAR and NM, and the cases must take the branches claimed: the cut in
    a match run and inside a deletion on either end, no fix, at least 4 regions each.  The regions of which nothing is left cannot be
    put to the reference (it ends the process, bwamem.c:1183-1186): their verdict is the restatement's over the oracle's alignment.
    cigar_golden.npz, the reference's recorded mem_reg2aln results, goes the same way on its one-sequence reference."""
    import kswlib
    import reflib
    import wantgen as wg
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    whole, pac = wg.reference()
    fa = str(tmp_path / "wg.fa")
    with open(fa, "w") as f:
        for k, (off, n) in enumerate(wg.CONTIGS):
            f.write(f">seq{k}\n" + "".join("ACGT"[b] for b in whole[off:off + n]) + "\n")
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac, rpac = reflib.pac_of(idx)
    assert l_pac == wg.L_PAC and bytes(rpac[:wg.L_PAC // 4]) == bytes(pac[:wg.L_PAC // 4])
    p = kswlib.make_params()
    opt = reflib.opt_from_params(p)
    seen = {k: 0 for k in ("Mb", "Me", "Db", "De", "none", "-2")}

    def one_try(rd, rb, re):
        rq = np.zeros((), kswlib.CIGAR_REQ)
        rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"] = 0, len(rd), rb, re, -100000, 100  # (infers more than opt->w: band 100)
        _, words, _, _, tries = kswlib.orc_reg2cigar(p, l_pac, pac, rd, rq)
        assert tries == 1
        return words
    for name, rd, reg, expect in wg.overhangs(whole):
        rb, re, qb, qe = int(reg["rb"]), int(reg["re"]), 0, len(rd)
        v, cb, ce = rp.xref_test(wg.CONTIGS, l_pac, rb, re)
        assert v == (expect != "none"), name
        took = {"none"}
        if v:
            words = one_try(rd, rb, re)
            took = rp.cut_branches(words, cb, ce, rb, re)
            verdict, qb, qe, rb, re = rp.xref_cut(words, cb, ce, qb, qe, rb, re)
            assert verdict == 0 and len(took) == 1, (name, took)
            if name[-1] == "+":  # (a hit on the reverse strand is aligned backwards and its CIGAR walked forwards, as the reference does)
                assert took == {expect}, (name, took)
        rq = np.zeros((), kswlib.CIGAR_REQ)
        rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"] = qb, qe, rb, re, int(reg["truesc"]), int(reg["w"])
        _, words, nm, md, _ = kswlib.orc_reg2cigar(p, l_pac, pac, rd, rq)
        fw, _ = kswlib.finish_aln(words, md, rq, len(rd), l_pac)
        n, rwords, rnm, rmd, ris_rev, rpos = reflib.ref_reg2aln(idx, opt, rd, reg)
        assert n == len(fw) and np.array_equal(fw, rwords) and nm == rnm, (name, fw, rwords, nm, rnm)
        assert _pos_of(rb, re, words, l_pac, wg.CONTIGS) == (rpos, ris_rev), (name, rpos, ris_rev)
        seen[took.pop()] += 1
    for name, rd, reg in wg.lost_regions(whole):
        rb, re = int(reg["rb"]), int(reg["re"])
        v, cb, ce = rp.xref_test(wg.CONTIGS, l_pac, rb, re)
        assert v == 1 and rp.xref_cut(one_try(rd, rb, re), cb, ce, 0, len(rd), rb, re)[0] == -2, name
        seen["-2"] += 1
    assert min(seen.values()) >= 4, seen
    n = 0
    for gp, gl, gpac, reads, reqs, exp in kswlib.golden_cigar_groups():  # one sequence: nothing hangs over, the coordinates stay
        for rq, (en, ew, enm, emd) in list(zip(reqs, exp))[::7]:
            assert rp.xref_test([(0, gl)], gl, int(rq["rb"]), int(rq["re"]))[0] == 0
            rd = reads[int(rq["read"])]
            _, words, nm, md, _ = kswlib.orc_reg2cigar(gp, gl, gpac, rd, rq)
            fw, fmd = kswlib.finish_aln(words, md, rq, len(rd), gl)
            assert len(fw) == en and np.array_equal(fw, ew) and nm == enm
            n += 1
    assert n >= 300


# ---------------------------------------------------------------- the interface

NEW = ("bmh_wanted_cigar_batch", "bmh_wanted_cigar_device", "bmh_ctx_set_refidx", "bmh_ctx_set_wanted_device", "bmh_last_wanted_stats")


def test_header_text_and_exported_symbols(pkg):
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    args = ("bmh_ctx_t *ctx, const bmh_refidx_t *bns, const uint8_t *pac, int w, int n, const bmh_read_t *reads, const bmh_alnreg_v *regs, "
            "const int64_t *roff, const int32_t *n_want, const int32_t *want_k, bmh_wanted_res_t *results, uint32_t *cigar_pool, size_t cigar_words, "
            "char *md_pool, size_t md_bytes);")
    assert "int bmh_wanted_cigar_batch(" + args in hdr
    assert "int bmh_wanted_cigar_device(" + args in hdr
    assert "int bmh_ctx_set_refidx(bmh_ctx_t *ctx, const bmh_refidx_t *bns);" in hdr
    assert "int bmh_ctx_set_wanted_device(bmh_ctx_t *ctx, int on);" in hdr
    assert "int bmh_last_wanted_stats(const bmh_ctx_t *ctx, int64_t *wanted, int64_t *fixed, int64_t *redone, float *kernel_ms);" in hdr
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    for name in ("bmh_wanted_host_", "bmh_wanted_deliver_", "bmh_wanted_routed_", "bmh_wanted_check_args_"):  # between the library's own files
        assert not hasattr(lib, name), name
    assert lib.bmh_version() == 310
    assert pkg.WANTED_RES.itemsize == 72
    assert callable(pkg.Context.wanted_cigar_batch) and callable(pkg.Context.set_refidx) and callable(pkg.Context.set_wanted_device)


def test_wanted_res_layout(pkg, tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    fields = ("rb", "re", "qb", "qe", "score", "n_cigar", "NM", "tries", "cigar_off", "md_off", "md_len", "flags", "band")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bwamem_hip.h"\nint main(void)\n{\n\tprintf("%zu", sizeof(bmh_wanted_res_t));\n'
                   + "".join(f'\tprintf(" %zu", offsetof(bmh_wanted_res_t, {f}));\n' for f in fields) + "\treturn 0;\n}\n")
    cc = subprocess.run([gcc, "-I" + os.path.dirname(pkg.HEADER_PATH), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [72] + [pkg.WANTED_RES.fields[f][1] for f in fields]


def test_refusals_without_a_context(pkg):
    lib = pkg.lib()
    idx = pkg.make_refidx(CONTIGS)
    pac = np.zeros(L_PAC // 4 + 1, dtype=np.uint8)
    tail = [None] * 7 + [C.c_size_t(0), None, C.c_size_t(0)]
    assert lib.bmh_wanted_cigar_device(None, C.byref(idx), pac.ctypes.data_as(C.c_void_p), 100, 0, *tail) == pkg.BMH_E_ARG
    assert lib.bmh_wanted_cigar_batch(None, C.byref(idx), pac.ctypes.data_as(C.c_void_p), 100, 0, *tail) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_refidx(None, C.byref(idx)) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_refidx(None, None) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_wanted_device(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_wanted_stats(None, None, None, None, None) == pkg.BMH_E_ARG
