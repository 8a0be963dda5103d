"""host/regfinish_core.h -- the replay of the band loop and the NM/MD walk the long round of bmh_region_cigar_batch_long runs per
flagged region -- on the CPU, as a stand-alone program (tests/regfinish_core_main.c) built once plainly and once under
AddressSanitizer, with every sequence and every output in a heap block of exactly its size.  On the regions of
tests/regionlonggen.py; expectations: the oracle's orc_reg2cigar (orc_gen_cigar for one-try requests), the generator's own reference (which the GPU tests use), and
where oracle/_ref exists the compiled reference's bwa_gen_cigar2."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kswlib
import regionlonggen as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "regfinish_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LINE = re.compile(r"region (\d+): bands (-?\d+) (-?\d+) (-?\d+) score (-?\d+) n_cigar (\d+) tries (\d+) fin (-?\d+) NM (-?\d+) md_len (\d+) "
                  r"sized (\d+) cigar (\S+) md (\S+)")


@pytest.fixture(scope="module")
def params():
    return kswlib.make_params()


@pytest.fixture(scope="module")
def cases(tmp_path_factory, params):
    path = tmp_path_factory.mktemp("rfin") / "regions.bin"
    _, pac, _ = gen.genome()
    p = np.ascontiguousarray(params, dtype=kswlib.PARAMS)
    assert p.nbytes == 64
    with open(path, "wb") as f:
        f.write(p.tobytes() + struct.pack("<qi", gen.L_PAC, len(pac)) + pac.tobytes() + struct.pack("<i", len(gen.regions())))
        for r in gen.regions():
            f.write(struct.pack("<i", len(r["read"])) + r["read"].tobytes() + struct.pack("<qqii", r["rb"], r["re"], r["truesc"], r["reg_w"]))
    return path


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    kswlib.load_oracle()  # liborc.so is there
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-L" + kswlib.ORACLE_DIR, "-lorc", "-Wl,-rpath," + kswlib.ORACLE_DIR],
                        capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    rows = LINE.findall(run.stdout)
    assert len(rows) == len(gen.regions()) and f"{len(rows)} regions, 0 differ" in run.stdout
    out = []
    for m in rows:
        out.append(dict(bands=[int(m[1]), int(m[2]), int(m[3])], score=int(m[4]), n_cigar=int(m[5]), tries=int(m[6]), fin=int(m[7]), NM=int(m[8]),
                        md_len=int(m[9]), sized=int(m[10]), words=np.array([int(x, 16) for x in m[11].split(",")], dtype=np.uint32),
                        md=b"" if m[12] == "-" else m[12].encode()))
    return out


def _oracle(params, pac, read, req):
    """(score, words, NM, MD, tries): orc_reg2cigar, or for a one-try request (truesc == INT32_MIN, which the oracle's loop does not
    know) its single call orc_gen_cigar on the band reg_w"""
    if int(req["truesc"]) != gen.INT_MIN:
        return kswlib.orc_reg2cigar(params, gen.L_PAC, pac, read, req)
    lib = kswlib.load_oracle()
    lib.orc_gen_cigar.restype = None
    pp = np.ascontiguousarray(np.asarray(params, dtype=kswlib.PARAMS).reshape(()))
    read = np.ascontiguousarray(read, dtype=np.uint8)
    o = kswlib._OrcCigar()
    lib.orc_gen_cigar(pp.ctypes.data_as(C.c_void_p), C.c_int(int(req["reg_w"])), C.c_int64(gen.L_PAC), pac.ctypes.data_as(C.c_void_p),
                      C.c_int(len(read)), read.ctypes.data_as(C.c_void_p), C.c_int64(int(req["rb"])), C.c_int64(int(req["re"])), C.byref(o))
    res = (o.score, np.array([o.cigar[i] for i in range(o.n_cigar)], dtype=np.uint32), o.NM, bytes(o.md) if o.md else b"", 1)
    lib.orc_cigar_free(C.byref(o))
    return res


def test_generator_covers_every_class(params):
    """From the oracle alone: CLASS_MIN regions CIGAR-cut, MD-cut, both, per strand and per final try; a ring region per strand; the
    named operation counts and edge cases."""
    c = gen.classes(params)
    print(c)
    gen.check_classes(c)


def test_header_equals_oracle_and_generator_reference(cases, tmp_path, params):
    _, exe, cc = _build(tmp_path, "rfin_plain", [])
    assert cc.returncode == 0, cc.stderr
    got = _run(exe, cases)
    _, pac, _ = gen.genome()
    reads, reqs = gen.cigar_reqs(list(range(len(gen.regions()))))
    for k, (g, r) in enumerate(zip(got, gen.regions())):
        ql, tl = len(r["read"]), r["re"] - r["rb"]
        assert g["bands"] == gen.plan(params, ql, tl, r["truesc"], r["reg_w"])[0], (k, g["bands"])  # the generator's plan is the header's
        oscore, owords, onm, omd, otries = _oracle(params, pac, reads[k], reqs[k])
        assert (g["score"], g["tries"], g["NM"], g["md"]) == (oscore, otries, onm, omd), (k, r["kind"], g, (oscore, otries, onm, omd))
        assert np.array_equal(g["words"], owords), (k, r["kind"])
        assert g["sized"] == g["md_len"] == len(omd) and g["n_cigar"] == len(owords)  # the size pass equals the bytes written
        x = gen.reference(params, k)  # what the GPU tests compare with
        assert (x["score"], x["tries"], x["NM"], x["md"], x["fin"]) == (oscore, otries, onm, omd, g["fin"]), (k, r["kind"])
        assert np.array_equal(x["words"], owords)


def test_header_equals_compiled_reference(cases, tmp_path, params):
    """bwa_gen_cigar2 of the compiled reference on the final try's band: the same CIGAR, NM and MD."""
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("the compiled reference (oracle/_ref) is not built")
    _, exe, cc = _build(tmp_path, "rfin_plain", [])
    assert cc.returncode == 0, cc.stderr
    got = _run(exe, cases)
    L = reflib.lib()
    L.bwa_gen_cigar2.restype = C.POINTER(C.c_uint32)
    L.bwa_gen_cigar2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_int64, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _, pac, _ = gen.genome()
    mat = np.ascontiguousarray(params["mat"], dtype=np.int8)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    n = 0
    for k, (g, r) in enumerate(zip(got, gen.regions())):
        read = np.ascontiguousarray(r["read"], dtype=np.uint8).copy()  # (reversed in place and back, bwa.c:102-107)
        w2 = gen.first_band(params, len(read), r["re"] - r["rb"], r["truesc"], r["reg_w"])
        w_try = w2 if g["fin"] < 0 else min(w2 << g["fin"], 2 ** 31 - 1)
        score, n_cigar, nm = C.c_int(0), C.c_int(0), C.c_int(0)
        cg = L.bwa_gen_cigar2(mat.ctypes.data, int(params["o_del"]), int(params["e_del"]), int(params["o_ins"]), int(params["e_ins"]), w_try,
                              gen.L_PAC, pac.ctypes.data, len(read), read.ctypes.data, r["rb"], r["re"], C.byref(score), C.byref(n_cigar),
                              C.byref(nm))
        assert cg, k
        words = np.array([cg[i] for i in range(n_cigar.value)], dtype=np.uint32)
        md = C.string_at(C.cast(cg, C.c_void_p).value + 4 * n_cigar.value)
        libc.free(C.cast(cg, C.c_void_p))
        assert (score.value, nm.value, md) == (g["score"], g["NM"], g["md"]) and np.array_equal(words, g["words"]), (k, r["kind"])
        n += 1
    assert n == len(gen.regions())


def test_header_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, exe, plain = _build(tmp_path, "rfin_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "rfin_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, cases)
