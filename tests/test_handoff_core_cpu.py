"""host/handoff_core.h on the CPU: the reduction table_plan_kernel makes over a batch's regions (and decide_table_sizes and oriented_cap
of csrc/api.hip make over a caller's vectors), as tests/handoff_core_main.c runs it -- per read, per group of 64, merged -- against a
plain Python restatement of the two host routines as they stood before the header (tests/handoff_ref.py), on seeded random vectors
with every clause in them: empty vectors, sub_n negative, seedcov negative (the refusal, only without mapQ_coef_len), lengths on both
sides of mapQ_coef_len, spans negative and past 65535.  Plainly, and under AddressSanitizer with every vector in a heap block of its
exact size."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import handoff_ref as hr
import kswlib
from test_postproc_cpu import sam_opt

SRC = os.path.join(kswlib.ROOT, "tests", "handoff_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
# (name, options, reads, seedcov < 0 among them)
CASES = [("default", dict(), 3000, False), ("default_negcov", dict(), 1500, True), ("seedcov", dict(mapQ_coef_len=0.0), 3000, False),
         ("seedcov_neg", dict(mapQ_coef_len=0.0), 1500, True), ("coef_len_300", dict(mapQ_coef_len=300.0), 700, False),
         ("one_read", dict(), 1, False), ("sixty_five", dict(mapQ_coef_len=0.0), 65, False), ("no_reads", dict(), 0, False)]


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-lm"], capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    print(run.stdout.strip())
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    m = re.fullmatch(r"reads (\d+) total (\d+) kmax (\d+) opool_cap (\d+) neg (\d+)\s*", run.stdout)
    assert m, run.stdout
    return tuple(int(x) for x in m.groups())


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per case (name, file, options, vectors, the restatement's answer)"""
    d = tmp_path_factory.mktemp("handoff_cases")
    out = []
    for k, (name, kw, n, neg) in enumerate(CASES):
        o = sam_opt(**kw)
        vecs = hr.random_vectors(np.random.default_rng(4100 + k), n, neg_seedcov=neg)
        path = d / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(np.array([0x48414e44, n], dtype="<i4").tobytes())
            f.write(o.tobytes())
            f.write(np.array([len(v) for v in vecs], dtype="<i4").tobytes())
            f.write(np.concatenate([np.zeros(0, dtype=hr.ALNREG)] + vecs).tobytes())
        out.append((name, path, o, vecs, hr.plan(o, vecs)))
    return out


def _check(exe, cases):
    for name, path, o, vecs, (kmax, cap, total, refused) in cases:
        n, got_total, got_kmax, got_cap, got_neg = _run(exe, path)
        assert (n, got_total, got_cap, got_neg) == (len(vecs), total, cap, int(refused)), name
        if not refused:  # (decide_table_sizes returns at the first negative index: it has no kmax then)
            assert got_kmax == kmax, name


def test_the_inputs_hold_every_clause(cases):
    by = {name: (o, vecs, want) for name, _, o, vecs, want in cases}
    _, vecs, (kmax, cap, total, refused) = by["default"]
    flat = np.concatenate(vecs)
    ql, rl = flat["qe"].astype(np.int64) - flat["qb"], flat["re"] - flat["rb"]
    assert sum(len(v) == 0 for v in vecs) > 300 and max(len(v) for v in vecs) == 40
    assert (flat["sub_n"] < 0).sum() > 500 and (flat["sub_n"] > 65_535).sum() > 100
    assert (ql < 0).sum() > 500 and (rl < 0).sum() > 500 and (ql > 65_535).sum() > 100 and (rl > 65_535).sum() > 100
    assert (ql == 65_535).sum() + (ql == 65_534).sum() > 0
    lens = np.array([hr.pp_len(a) for a in flat[:4000]])
    assert (lens < 0).sum() > 50 and ((lens >= 0) & (lens < 50)).sum() > 50 and (lens >= 50).sum() > 1000
    assert not refused and kmax > 70_000 and cap > 65_535 * 200 and total == len(flat)
    # seedcov < 0 is the refusal exactly where the index is seedcov
    assert by["default_negcov"][2][3] is False and (np.concatenate(by["default_negcov"][1])["seedcov"] < 0).sum() > 20
    assert by["seedcov_neg"][2][3] is True and by["seedcov"][2][3] is False
    assert by["no_reads"][2] == (1, 0, 0, False) and by["one_read"][2][2] == len(by["one_read"][1][0])


def test_core_program_matches_the_restatement(cases, tmp_path):
    _, exe, cc = _build(tmp_path, "ho_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    assert cc.stderr.strip() == "", cc.stderr  # -Wall clean
    _check(exe, cases)


def test_core_program_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, _, plain = _build(tmp_path, "ho_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "ho_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _check(exe, cases)


def test_api_is_built_on_the_header():
    """decide_table_sizes and oriented_cap hold no rule of their own any more: host and device cannot drift apart"""
    api = open(os.path.join(kswlib.ROOT, "bwa-mem-quickassist_amd", "csrc", "api.hip")).read()
    c2r = open(os.path.join(kswlib.ROOT, "bwa-mem-quickassist_amd", "csrc", "chain2reg.hip")).read()
    assert '#include "../host/handoff_core.h"' in api and '#include "../host/handoff_core.h"' in c2r
    body = api[api.index("static int decide_table_sizes("):api.index("static int decide_host_log(")]
    assert "bmh_ho_read(" in body and "bmh_ho_pair_kmax(" in body and "mapQ_coef_len" not in body and "seedcov" not in body
    assert "static size_t oriented_cap(const bmh_alnreg_t *a) { return (size_t)bmh_ho_oriented_cap(a); }" in api
    assert "bmh_ho_read(&o, reg + at" in c2r and c2r.count("bmh_ho_read(") == 1  # one plan kernel, for the workspace and for any table
