"""host/extstop_core.h -- when a ksw_extend2 flank may end before the reference's loop does -- as a stand-alone program
(tests/extstop_core_main.c: a plain restatement of ksw_extend2 with the rule taken from the header) built once plainly and once under
AddressSanitizer, every sequence in a heap block of exactly its length.  With the rule per cell and per block of eight columns, all six
outputs must be the oracle's; without it, the rows and cells as well.  The block form's rows per task must also be those of the Python
restatement the GPU test reads the kernels' rows against (tests/extstop_ref.py)."""
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import extstop_cases as xc
import extstop_ref
import kswgen
import kswlib
from __graft_entry__ import load_package

SRC = os.path.join(kswlib.ROOT, "tests", "extstop_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LINE = re.compile(r"case (\d+): (\d+) tasks, (\d+) differ, (\d+) order errors, (\d+) cut, rows (\d+) (\d+) (\d+), cells (\d+) (\d+) (\d+)")
ROWS = re.compile(r"rows (\d+):([ \d]*)")

DEFAULT = dict()
SCORINGS = {"default": dict(), "open0": dict(o_del=0, o_ins=0), "asym": dict(o_del=6, e_del=1, o_ins=4, e_ins=2),
            "a3": dict(a=3, b=4, o_del=5, e_del=2, o_ins=5, e_ins=2), "zdrop5": dict(zdrop=5), "zdrop20": dict(zdrop=20), "zdrop0": dict(zdrop=0)}


def _taskgen():
    return importlib.import_module(load_package().__name__ + ".taskgen")


def _write_case(f, p, mode, pool, tasks):
    p = np.ascontiguousarray(p, dtype=kswlib.PARAMS)
    tasks = np.ascontiguousarray(tasks, dtype=kswlib.EXT_TASK)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    f.write(p.tobytes() + struct.pack("<iq", mode, len(pool)) + pool.tobytes() + struct.pack("<i", len(tasks)) + tasks.tobytes())


def _targeted():
    rng = np.random.default_rng(41)
    parts, kinds = [], []
    for L in (1, 2, 7, 8, 9, 31, 33, 64, 100, 128, 150):
        pool, tasks, k = xc.targeted(rng, L)
        parts.append((pool, tasks))
        kinds += k
    parts.append(xc.tiny(rng))
    kinds += ["tiny"] * len(parts[-1][1])
    return xc.merge(parts) + (kinds,)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the input file, the cases' names in order, {name: (params, pool, tasks)} of the cases whose rows are printed)"""
    tg = _taskgen()
    rng = np.random.default_rng(11)
    p0 = kswlib.make_params()
    gen = tg.generate(p0, 20000, "150bp", seed=7)[:2]
    mixed = tg.generate(p0, 1500, "mixed100-300", seed=7)[:2]
    tpool, ttasks, _ = _targeted()
    fuzz = kswgen.gen_ext_fuzz(rng, 3000, p0)
    hard = kswgen.gen_ext_realistic(rng, 1500, (100, 250), hard=True)
    sets = [("gen150", DEFAULT, 0, gen), ("mixed", DEFAULT, 0, mixed), ("fuzz", DEFAULT, 0, fuzz), ("hard", DEFAULT, 0, hard)]
    printed = {}
    for name, kw in SCORINGS.items():
        sets.append((name + "/targeted", kw, 2, (tpool, ttasks)))
        printed[name + "/targeted"] = (kswlib.make_params(**kw), tpool, ttasks)
        sets.append((name + "/fuzz", kw, 0, (fuzz[0], fuzz[1][:1000])))
    sets.append(("gen150/head", DEFAULT, 2, (gen[0], gen[1][:1200])))
    printed["gen150/head"] = (p0, gen[0], gen[1][:1200])
    # a matrix without a non-negative entry: the rule must leave every task alone
    sets.append(("A<0", dict(mat=np.minimum(kswlib.fill_scmat(1, 4), -1)), 0, (tpool, ttasks)))
    path = tmp_path_factory.mktemp("extstop") / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(sets)))
        for _, kw, mode, (pool, tasks) in sets:
            _write_case(f, kswlib.make_params(**kw), mode, pool, tasks)
    return path, [s[0] for s in sets], printed



def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    kswlib.load_oracle()  # liborc.so is there
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-L" + kswlib.ORACLE_DIR, "-lorc", "-Wl,-rpath," + kswlib.ORACLE_DIR],
                        capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, args, names=None):
    run = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True)
    rows = [tuple(int(x) for x in m) for m in LINE.findall(run.stdout)]
    names = names or [str(r[0]) for r in rows]
    print("\n".join(f"{n}: {r}" for n, r in zip(names, rows)))  # every figure, before anything is asserted
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert rows and len(rows) == len(names) and all(r[2] == 0 and r[3] == 0 for r in rows), rows
    per_task = {int(c): [int(x) for x in v.split()] for c, v in ROWS.findall(run.stdout)}
    return dict(zip(names, rows)), per_task


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    _, exe, cc = _build(tmp_path_factory.mktemp("xs_plain"), "xs_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    return exe


def test_every_short_pair_over_two_letters(plain):
    """query <= 5, target <= 8, h0 in {0,1,3,9}, w in {1,2,100}, zdrop in {0,2,100}, six scorings: 6.8 M tasks, three forms each."""
    rows, _ = _run(plain, ["exhaustive", 5, 8])
    assert len(rows) == 6 and all(r[1] == 1138320 for r in rows.values())
    assert all(r[6] < r[5] for r in rows.values()), "the per-cell form never fired: nothing was compared"


def test_random_related_pairs(plain):
    rows, _ = _run(plain, ["random", 400000, 20261019])
    (r,) = rows.values()
    assert r[1] == 400000 and r[4] > 40000 and r[7] < r[5], r  # the block form cut a good part: those were compared with the oracle


def test_generator_and_targeted_tasks_and_the_rule_bites(plain, cases):
    path, names, printed = cases
    rows, per_task = _run(plain, ["file", path], names)
    # where the rule does not apply, every form runs the reference's rows
    assert rows["A<0"][4] == 0 and rows["A<0"][5] == rows["A<0"][6] == rows["A<0"][7]
    for name in SCORINGS:
        assert rows[name + "/targeted"][4] > 0, (name, rows[name + "/targeted"])
    # the rows the C program got from the header == the Python restatement's, task by task
    for name, (p, pool, tasks) in printed.items():
        got = np.array(per_task[names.index(name)])
        want, out = extstop_ref.rows(p, pool, tasks)
        orc, _ = kswlib.orc_extend_batch(p, pool, tasks)
        assert (out == orc).all(), name + ": the Python restatement's outputs differ from the oracle's"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{name}: rows differ for {len(bad)} tasks; first {bad[0]}: header {got[bad[0]]} python {want[bad[0]]} task {tasks[bad[0]]}"
    # the rule has not decayed into a no-op: the bench's own task set (0.773 of the cells, 97.9 % of the tasks cut)
    _, n, _, _, cut, r0, _, r2, c0, _, c2 = rows["gen150"]
    print(f"gen150: {n} tasks, rows per task {r0 / n:.1f} -> {r2 / n:.1f}, cells x {c2 / c0:.4f}, cut {cut / n:.4f}")
    assert c2 <= 0.80 * c0 and cut >= 0.95 * n, (c0, c2, cut, n)


def test_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, exe, plain = _build(tmp_path, "xs_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "xs_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, ["exhaustive", 4, 5])
    _run(exe, ["random", 20000, 5])
    small = tmp_path / "small.bin"
    tpool, ttasks, _ = _targeted()
    with open(small, "wb") as f:
        f.write(struct.pack("<i", len(SCORINGS)))
        for kw in SCORINGS.values():
            _write_case(f, kswlib.make_params(**kw), 0, tpool, ttasks)
    _run(exe, ["file", small], list(SCORINGS))
