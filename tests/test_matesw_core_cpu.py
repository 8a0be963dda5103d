"""host/matesw_core.h -- the rules the two mate-rescue drivers share -- driven on the CPU exactly as the device loop of csrc/matesw.hip
drives them (fold, plan, append; the oracle's ksw_align2 in place of the kernels), as a stand-alone program (tests/matesw_core_main.c)
built once plainly and once under AddressSanitizer, with every vector in a heap block of exactly its slice capacity and every range
stack of exactly bmh_sort_stack_len(n) entries.  Expectations: the committed fixture's (the compiled reference's own loop), and on the
generated batches of tests/mswgen.py the oracle's orc_matesw_pair given bmh_dedup_core as its mem_sort_and_dedup."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kswlib
import mswgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "matesw_core_main.c")
LOOKAHEAD = 8  # BMH_MSW_LOOKAHEAD, host/matesw_core.h
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

# (batch, scoring, table, option set) of the generated cases, the all-open default run first
GENERATED = [("main", "byte", "all", "default"), ("main", "word", "fr", "default"), ("main", "byte", "fr", "default"),
             ("main", "byte", "all", "three"), ("main", "byte", "fr", "one"), ("main", "byte", "fr", "best_only"),
             ((65, 40), "byte", "fr", "default"), ((0, 30), "byte", "fr", "default"), ((1, 9), "byte", "none", "default")]


def _case(f, p, o, pes, level, mode, l_pac, pac, reads, regs, exp=None, n_sw=None):
    p = np.ascontiguousarray(p, dtype=kswlib.PARAMS)
    o = np.ascontiguousarray(o, dtype=kswlib.MATESW_OPT)
    pes = np.ascontiguousarray(pes, dtype=kswlib.PESTAT)
    pac = np.ascontiguousarray(pac, dtype=np.uint8)
    assert p.nbytes == 64 and o.nbytes == 16 and pes.nbytes == 128
    f.write(p.tobytes() + o.tobytes() + pes.tobytes() + struct.pack("<fiqi", level, mode, l_pac, len(pac)) + pac.tobytes())
    f.write(struct.pack("<i", len(reads) // 2))
    for r in reads:
        r = np.ascontiguousarray(r, dtype=np.uint8)
        f.write(struct.pack("<i", len(r)) + r.tobytes())
    for vs in (regs, exp) if mode == 0 else (regs,):
        for v in vs:
            v = np.ascontiguousarray(v, dtype=kswlib.ALNREG)
            f.write(struct.pack("<i", len(v)) + v.tobytes())
    if mode == 0:
        f.write(np.asarray(n_sw, dtype="<i4").tobytes())


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the input file, number of fixture cases)"""
    path = tmp_path_factory.mktemp("msw") / "cases.bin"
    g = kswlib.load_golden("matesw_golden.npz")
    groups = list(kswlib.golden_matesw_groups())
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(groups) + len(GENERATED)))
        for key, (p, o, pes, l_pac, pac, reads, regs, exp, n_sw) in zip(g["groups"], groups):
            _case(f, p, o, pes, float(g[str(key) + "mask_level_redun"]), 0, l_pac, pac, reads, regs, exp, n_sw)
        l_pac, pac, _ = mswgen.genome()
        for batch, sc, table, opt in GENERATED:
            reads, regs = mswgen.main_batch(sc) if batch == "main" else mswgen.mixed_batch(*batch)
            _case(f, mswgen.scoring(sc), mswgen.opt(opt), mswgen.pes(table), mswgen.LEVEL, 1, l_pac, pac, reads, regs)
    return path, len(groups)


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    kswlib.load_oracle()  # liborc.so is there
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-L" + kswlib.ORACLE_DIR, "-lorc", "-Wl,-rpath," + kswlib.ORACLE_DIR],
                        capture_output=True, text=True)
    return gcc, exe, cc


LINE = re.compile(r"case (\d+): (\d+) pairs, (\d+) active, (\d+) rounds, (\d+) tasks, (\d+) empty-window plans, (\d+) no-call plans, "
                  r"(\d+) needed-after-all stops, (\d+) differ")


def _run(exe, cases):
    path, n_fix = cases
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    print(run.stdout)  # every figure, before anything is asserted
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-4000:]}"
    rows = [tuple(int(x) for x in m) for m in LINE.findall(run.stdout)]
    assert len(rows) == n_fix + len(GENERATED) and all(r[-1] == 0 for r in rows), run.stdout
    return rows[:n_fix], rows[n_fix:]


def test_the_generated_batches_reach_new_ground():
    """On the oracle's side of the main batch: second rounds, vectors grown from nothing, regions for mem_sort_and_dedup to remove."""
    reads, regs = mswgen.main_batch("byte")
    _, ns, _ = mswgen.oracle("main", "byte", "fr", "default")
    assert sum(n > LOOKAHEAD for n in ns) >= 40, ns  # under FR only an invocation is one call
    want, ns, removed = mswgen.oracle("main", "byte", "all", "default")
    assert max(len(w) for w, r in zip(want, regs) if len(r) == 0) >= 10
    assert removed >= 10 and sum(n > 32 for n in ns) >= 20, (removed, ns)


def test_shared_routines_reproduce_fixture_and_oracle(cases, tmp_path):
    _, exe, cc = _build(tmp_path, "msw_plain", [])
    assert cc.returncode == 0, cc.stderr
    fix, gen = _run(exe, cases)
    assert sum(r[4] for r in fix) > 4000  # the fixture's ksw_align2 calls
    # the all-open run of the main batch: several rounds, and every plan code occurs
    _, pairs, active, rounds, tasks, empty, nocall, _needed, _ = gen[0]
    assert pairs == 104 and active == 104 and rounds >= 2 and tasks > 3000 and empty > 0 and nocall > 0, gen[0]
    assert gen[2][3] >= 2, gen[2]  # FR only: a second round
    by = dict(zip([tuple(map(str, g)) for g in GENERATED], gen))
    assert by[("(65, 40)", "byte", "fr", "default")][2] == 65 and by[("(0, 30)", "byte", "fr", "default")][2] == 0
    assert by[("(1, 9)", "byte", "none", "default")][2:5] == (0, 0, 0)  # all four orientations failed: nothing to do


def test_shared_routines_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, exe, plain = _build(tmp_path, "msw_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "msw_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, cases)
