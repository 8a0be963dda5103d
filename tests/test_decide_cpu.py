"""Pass A of phase 2 as one batch call on the host, bmh_decide_batch (host/sam_post.c over host/postproc_core.h): primary marking,
pairing, the tail of mem_sam_pe, the selection of mem_reg2sam_se and mem_approx_mapq_se of every region.
 * single-end: the committed fixture of the compiled reference (tests/golden/postproc_golden.npz) under its four option sets;
 * paired-end: the composition of the single routines the fixture pins (bmh_mark_primary_se, bmh_pair) and a Python restatement of
   the selection, also at read ids where mem_pair's `(int)id << 8` truncates, and there live against the reference where it is built;
 * the core as a stand-alone program (tests/decide_core_main.c), plainly and under AddressSanitizer with every block of exactly
   its size, must print the records the library computes."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import decidegen as dg
import kswlib
import postgen
from __graft_entry__ import load_package
from test_postproc_cpu import L  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "decide_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.mark.parametrize("si", range(len(postgen.OPTION_SETS)))
def test_single_end_reproduces_the_reference_fixture(pkg, si):
    o, vecs, marked, mapq = dg.se_fixture(si)
    out = pkg.decide_batch(o, dg.L_PAC, None, dg.SE_ID0, dg.se_spread(vecs))
    got = np.concatenate(out["regs"])
    assert got.tobytes() == np.ascontiguousarray(marked, dtype=kswlib.ALNREG).tobytes(), f"set {si}: the marked vectors differ"
    assert (out["reg_mapq"] == mapq).all(), f"set {si}: mapQ differs at {np.nonzero(out['reg_mapq'] != mapq)[0][:8]}"
    for i, a in enumerate(out["regs"]):
        assert list(out["want"][i]) == dg.want_se_py(o, a), i
    assert len(out["pd"]) == 0 and sum(len(w) for w in out["want"]) > 100


@pytest.mark.parametrize("si", range(len(postgen.OPTION_SETS)))
def test_paired_end_is_the_composition_of_the_single_routines(pkg, L, si):  # noqa: F811
    o, pes = dg.pe_opt(si), dg.fixture_pes(si)
    vecs = dg.pe_vectors(500 + si, 400)
    out = pkg.decide_batch(o, dg.L_PAC, pes, 2000, vecs)
    n_paired, n_won = dg.check_pe_composition(L, o, dg.L_PAC, pes, 2000, vecs, out)
    assert n_paired > 100 and n_won > 50 and n_paired > n_won, (n_paired, n_won)  # both outcomes of a paired decision occur
    assert (out["pd"]["q_pe"][out["pd"]["paired"] == 0] == 0).all()
    assert (out["pd"]["n_sub"] > 0).sum() > 5


@pytest.mark.parametrize("flag", [dg.NOPAIRING, dg.ALL, dg.NOPAIRING | dg.ALL])
def test_paired_end_flags(pkg, L, flag):  # noqa: F811
    o, pes = dg.pe_opt(0, flag), dg.fixture_pes(0)
    vecs = dg.pe_vectors(77, 200)
    out = pkg.decide_batch(o, dg.L_PAC, pes, 0, vecs)
    n_paired, _ = dg.check_pe_composition(L, o, dg.L_PAC, pes, 0, vecs, out)
    assert (n_paired == 0) == bool(flag & dg.NOPAIRING)
    if flag & dg.ALL:  # secondary hits get printed
        assert any(int(a[k]["secondary"]) >= 0 for a, w in zip(out["regs"], out["want"]) for k in w)


@pytest.mark.parametrize("id0", dg.ID0_TRUNCATING)
def test_ids_where_mem_pair_truncates(pkg, L, id0):  # noqa: F811
    o, pes = dg.pe_opt(0), dg.fixture_pes(0)
    vecs = dg.pe_vectors(9, 60)
    out = pkg.decide_batch(o, dg.L_PAC, pes, id0, vecs)
    n_paired, _ = dg.check_pe_composition(L, o, dg.L_PAC, pes, id0, vecs, out)
    assert n_paired > 10


@pytest.mark.ref
@pytest.mark.parametrize("id0", dg.ID0_TRUNCATING)
def test_ids_where_mem_pair_truncates_against_the_live_reference(pkg, id0):
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    R = reflib.lib()
    R.mem_mark_primary_se.restype = None
    R.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    R.mem_approx_mapq_se.restype = C.c_int
    R.mem_approx_mapq_se.argtypes = [C.c_void_p, C.c_void_p]
    R.mem_pair.restype = C.c_int
    opt = R.mem_opt_init()
    o, pes = dg.pe_opt(0), dg.fixture_pes(0)
    vecs = dg.pe_vectors(9, 60)
    out = pkg.decide_batch(o, dg.L_PAC, pes, id0, vecs)
    for p in range(len(vecs) // 2):
        pid = (id0 >> 1) + p
        m = []
        for r in range(2):
            a = vecs[2 * p + r].copy()
            if len(a):
                R.mem_mark_primary_se(opt, len(a), a.ctypes.data_as(C.c_void_p), C.c_int64(pid << 1 | r))
            m.append(a)
        d = out["pd"][p]
        if len(m[0]) and len(m[1]):
            c_regs = kswlib.regs_to_c(m)
            sub, nsub = C.c_int(0), C.c_int(0)
            z = (C.c_int * 2)(-1, -1)
            oo = R.mem_pair(opt, C.c_int64(dg.L_PAC), None, pes.ctypes.data_as(C.c_void_p), None, c_regs, C.c_int(((pid & 0xffffffff) ^ 0x80000000) - 0x80000000),
                            C.byref(sub), C.byref(nsub), z)
            kswlib.regs_from_c(c_regs)
            assert (int(d["score"]), int(d["sub"]), int(d["n_sub"])) == (oo, sub.value, nsub.value), (p, d)
            if oo > 0 and not (int(d["paired"]) and not int(d["extra_flag"]) & 2):
                assert tuple(d["z"]) == (z[0], z[1]), (p, d)
        for r in range(2):
            a = out["regs"][2 * p + r]
            if not (int(d["paired"]) and int(d["extra_flag"]) & 2):
                assert a.tobytes() == m[r].tobytes(), (p, r)
            for k in range(len(a)):
                assert R.mem_approx_mapq_se(opt, a[k:k + 1].ctypes.data_as(C.c_void_p)) == out["reg_mapq"][sum(len(v) for v in vecs[:2 * p + r]) + k]


def test_bad_arguments(pkg):
    o = dg.pe_opt(0)
    vecs = dg.pe_vectors(9, 3)
    with pytest.raises(pkg.BmhError) as e:
        pkg.decide_batch(o, dg.L_PAC, dg.fixture_pes(0), 0, vecs[:5])  # odd n with PE
    assert e.value.code == -3
    roff = np.cumsum([0] + [len(v) for v in vecs])
    roff[2] += 1
    with pytest.raises(pkg.BmhError) as e:
        pkg.decide_batch(o, dg.L_PAC, dg.fixture_pes(0), 0, vecs, roff=roff)
    assert e.value.code == -3
    assert pkg.lib().bmh_decide_batch(None, 0, None, 0, 0, None, None, None, None, None, None) == -3
    out = pkg.decide_batch(o, dg.L_PAC, dg.fixture_pes(0), 0, [])
    assert len(out["pd"]) == 0


# ---------------------------------------------------------------- the core as a stand-alone program

def _cases():
    """(options, pes or None, l_pac, id0, vectors) per case: the SE fixture of every option set, PE batches of every option set and
    flag, the truncating ids, vectors at the borders of the sort's paths, the special tables"""
    cs = []
    for si in range(len(postgen.OPTION_SETS)):
        o, vecs, _, _ = dg.se_fixture(si)
        cs.append((o, None, dg.L_PAC, dg.SE_ID0, dg.se_spread(vecs)[:7 * 150]))
        cs.append((dg.pe_opt(si), dg.fixture_pes(si), dg.L_PAC, 2000, dg.pe_vectors(500 + si, 120)))
    for flag in (dg.NOPAIRING, dg.ALL, dg.NOPAIRING | dg.ALL):
        cs.append((dg.pe_opt(0, flag), dg.fixture_pes(0), dg.L_PAC, 0, dg.pe_vectors(77, 60)))
    for id0 in dg.ID0_TRUNCATING:
        cs.append((dg.pe_opt(0), dg.fixture_pes(0), dg.L_PAC, id0, dg.pe_vectors(9, 60)))
    sizes = dg.vectors_of_sizes(np.random.default_rng(3), [0, 1, 2, 16, 17, 33, 40, 40, 33, 17, 16, 2, 1, 0])
    cs.append((dg.sam_opt(), None, 3_000_000, 5, sizes))
    cs.append((dg.pe_opt(2), dg.fixture_pes(2), 3_000_000, 6, sizes))
    for kind in ("none", "std0"):
        cs.append((dg.pe_opt(0), dg.special_pes(kind), dg.L_PAC, 10, dg.pe_vectors(21, 60)))
    return cs


@pytest.fixture(scope="module")
def program_input(tmp_path_factory):
    path = tmp_path_factory.mktemp("decide") / "cases.bin"
    cs = _cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for o, pes, l_pac, id0, vecs in cs:
            pes = np.zeros(4, dtype=kswlib.PESTAT) if pes is None else np.ascontiguousarray(pes, dtype=kswlib.PESTAT)
            assert o.nbytes == 96 and pes.nbytes == 128
            f.write(o.tobytes() + pes.tobytes() + struct.pack("<qqii", l_pac, id0, len(vecs), 0))
            for v in vecs:
                f.write(struct.pack("<i", len(v)) + np.ascontiguousarray(v, dtype=kswlib.ALNREG).tobytes())
    return path, cs


def _expected(pkg, cs):
    """what the program must print, from bmh_decide_batch"""
    lines = []
    for c, (o, pes, l_pac, id0, vecs) in enumerate(cs):
        out = pkg.decide_batch(o, l_pac, pes, id0, vecs)
        lines.append(f"case {c}")
        off = np.concatenate([[0], np.cumsum([len(v) for v in vecs])])
        pe = bool(int(o["flag"]) & dg.PE)
        for i in range(len(vecs)):
            lo, hi = int(off[i]), int(off[i + 1])
            lines.append(f"R {i} {out['regs'][i].tobytes().hex()}")
            lines.append(f"M {i} {out['reg_mapq'][lo:hi].tobytes().hex()}")
            lines.append(f"W {i} {int(out['n_want'][i])} {out['want_k'][lo:hi].tobytes().hex()}")
            if pe and i & 1:
                lines.append(f"P {i >> 1} {out['pd'][i >> 1].tobytes().hex()}")
    return lines


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


def test_core_program_prints_the_librarys_records(pkg, program_input, tmp_path):
    path, cs = program_input
    _, exe, cc = _build(tmp_path, "decide_plain", [])
    assert cc.returncode == 0, cc.stderr
    got, want = _run(exe, path), [l.rstrip() for l in _expected(pkg, cs)]
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (bad[:5], got[bad[0]][:200], want[bad[0]][:200])


def test_core_program_under_sanitizer_with_exact_blocks(pkg, program_input, tmp_path):
    path, cs = program_input
    gcc, _, plain = _build(tmp_path, "decide_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "decide_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    got, want = _run(exe, path), [l.rstrip() for l in _expected(pkg, cs)]
    assert got == want
