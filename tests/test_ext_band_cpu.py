"""host/extband_core.h -- the band a ksw_extend2 flank needs for its six outputs -- as a stand-alone program
(tests/extband_core_main.c) built once plainly and once under AddressSanitizer, every sequence in a heap block of exactly its length:
the oracle at the task's own w and at the header's w_eff must give six equal outputs.  The header's band must also be that of the
Python restatement the GPU test reads the device's bands against (tests/extband_ref.py), task by task, and the rule must still bite
on the bench's own task set."""
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import extband_cases as bc
import extband_ref
import extstop_cases as xc
import kswgen
import kswlib
from __graft_entry__ import load_package

SRC = os.path.join(kswlib.ROOT, "tests", "extband_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LINE = re.compile(r"case (\d+): (\d+) tasks, (\d+) differ, (\d+) narrowed, bands (\d+), cells (\d+) (\d+)")
BANDS = re.compile(r"bands (\d+):([ \d]*)")

DEFAULT = dict()
# the scorings of test_ext_stop_cpu.py, and a zero gap extension on both sides and on one
SCORINGS = {"default": dict(), "open0": dict(o_del=0, o_ins=0), "asym": dict(o_del=6, e_del=1, o_ins=4, e_ins=2),
            "a3": dict(a=3, b=4, o_del=5, e_del=2, o_ins=5, e_ins=2), "zdrop5": dict(zdrop=5), "zdrop20": dict(zdrop=20), "zdrop0": dict(zdrop=0),
            "e0": dict(e_del=0, e_ins=0), "e0del": dict(o_del=3, e_del=0)}


def _taskgen():
    return importlib.import_module(load_package().__name__ + ".taskgen")


def _write_case(f, p, mode, pool, tasks):
    p = np.ascontiguousarray(p, dtype=kswlib.PARAMS)
    tasks = np.ascontiguousarray(tasks, dtype=kswlib.EXT_TASK)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    f.write(p.tobytes() + struct.pack("<iq", mode, len(pool)) + pool.tobytes() + struct.pack("<i", len(tasks)) + tasks.tobytes())


def _targeted():
    rng = np.random.default_rng(43)
    parts = [xc.targeted(rng, L)[:2] for L in (1, 2, 7, 8, 9, 31, 33, 64, 100, 128, 150)]
    parts.append(xc.tiny(rng))
    parts.append(bc.handmade(rng)[:2])
    parts.append(bc.boundary(rng)[:2])
    return xc.merge(parts)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the input file, the cases' names in order, {name: (params, pool, tasks)} of the cases whose bands are printed)"""
    tg = _taskgen()
    rng = np.random.default_rng(12)
    p0 = kswlib.make_params()
    gen = tg.generate(p0, 20000, "150bp", seed=7)[:2]
    gen250 = tg.generate(p0, 1500, "250bp", seed=7)[:2]
    mixed = tg.generate(p0, 1500, "mixed100-300", seed=7)[:2]
    tpool, ttasks = _targeted()
    fuzz = kswgen.gen_ext_fuzz(rng, 3000, p0)
    hard = kswgen.gen_ext_realistic(rng, 1500, (100, 250), hard=True)
    sets = [("gen150", DEFAULT, 0, gen), ("gen250", DEFAULT, 0, gen250), ("mixed", DEFAULT, 0, mixed), ("fuzz", DEFAULT, 0, fuzz),
            ("hard", DEFAULT, 0, hard)]
    printed = {}
    for name, kw in SCORINGS.items():
        sets.append((name + "/targeted", kw, 2, (tpool, ttasks)))
        printed[name + "/targeted"] = (kswlib.make_params(**kw), tpool, ttasks)
        sets.append((name + "/fuzz", kw, 0, (fuzz[0], fuzz[1][:1000])))
    sets.append(("gen150/head", DEFAULT, 2, (gen[0], gen[1][:1200])))
    printed["gen150/head"] = (p0, gen[0], gen[1][:1200])
    sets.append(("mixed/head", DEFAULT, 2, (mixed[0], mixed[1][:600])))
    printed["mixed/head"] = (p0, mixed[0], mixed[1][:600])
    # a matrix without a non-negative entry: the rule must leave every task alone
    sets.append(("A<0", dict(mat=np.minimum(kswlib.fill_scmat(1, 4), -1)), 0, (tpool, ttasks)))
    path = tmp_path_factory.mktemp("extband") / "cases.bin"
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
    assert rows and len(rows) == len(names) and all(r[2] == 0 for r in rows), rows
    per_task = {int(c): [int(x) for x in v.split()] for c, v in BANDS.findall(run.stdout)}
    return dict(zip(names, rows)), per_task


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    _, exe, cc = _build(tmp_path_factory.mktemp("xb_plain"), "xb_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    return exe


def test_every_short_pair_over_two_letters(plain):
    """query <= 5, target <= 8, h0 in {0,1,3,6,8,9,12,20}, w in {1,2,3,100}, zdrop in {0,2,12,100}, eight scorings: 32 M tasks."""
    rows, _ = _run(plain, ["exhaustive", 5, 8])
    assert len(rows) == 8 and all(r[1] == 4047360 for r in rows.values())
    assert all(r[3] > 100000 and r[6] < r[5] for r in rows.values()), "the rule narrowed (almost) nothing: nothing was compared"


def test_random_related_pairs(plain):
    rows, _ = _run(plain, ["random", 400000, 20261019])
    (r,) = rows.values()
    assert r[1] == 400000 and r[3] > 40000 and r[6] < r[5], r  # a good part was narrowed: those were compared with the oracle


def test_generator_fuzz_and_handmade_tasks_and_the_rule_bites(plain, cases):
    path, names, printed = cases
    rows, per_task = _run(plain, ["file", path], names)
    assert rows["A<0"][3] == 0 and rows["A<0"][5] == rows["A<0"][6]  # where the rule does not apply, every task is left alone
    for name in SCORINGS:  # (zdrop = 5 is below o + e = 7: condition 5 can never hold, so nothing may be narrowed there)
        assert (rows[name + "/targeted"][3] > 0) == (name != "zdrop5"), (name, rows[name + "/targeted"])
    # the band the C program got from the header == the Python restatement's, task by task
    for name, (p, pool, tasks) in printed.items():
        got = np.array(per_task[names.index(name)])
        want = extband_ref.w_eff(p, pool, tasks)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{name}: bands differ for {len(bad)} tasks; first {bad[0]}: header {got[bad[0]]} python {want[bad[0]]} task {tasks[bad[0]]}"
    # the rule has not decayed: the bench's own task set (65.7 % of the tasks narrowed, 0.567 of the cells)
    _, n, _, narrowed, bands, c0, c1 = rows["gen150"]
    print(f"gen150: {n} tasks, narrowed {narrowed / n:.4f} (mean band {bands / max(narrowed, 1):.2f}), cells x {c1 / c0:.4f}")
    for name in ("gen250", "mixed"):
        print(f"{name}: narrowed {rows[name][3] / rows[name][1]:.4f}, cells x {rows[name][6] / rows[name][5]:.4f}")
    assert narrowed >= 0.55 * n and c1 <= 0.65 * c0, (n, narrowed, c0, c1)


def test_handmade_classes_and_both_sides_of_every_condition():
    """the two classes that broke earlier forms of the rule, and tasks one unit on either side of conditions 1-5: what the rule says of
    each, and six equal outputs from the oracle at w and at that band"""
    rng = np.random.default_rng(44)
    p = kswlib.make_params()
    pool, tasks, at = bc.handmade(rng)
    we = extband_ref.w_eff(p, pool, tasks)
    assert we[at] == tasks["w"][at] == 32, "condition 4 leaves the transient-gscore task alone"
    orc, _ = kswlib.orc_extend_batch(p, pool, tasks)
    assert tuple(orc[at]) == (15, 3, 3, 1, 0, 0)
    low = tasks["h0"] <= 1
    assert low.sum() >= 120 and (we[low] == tasks["w"][low]).all(), "h0 in {0, 1} is below every G: left alone"
    pool, tasks, idx = bc.boundary(rng)
    we = extband_ref.w_eff(p, pool, tasks)
    for name, (a, band, b) in idx.items():
        assert we[a] == band < tasks["w"][a], (name, we[a], band)
        if name == "2":
            assert we[b] == 2, (name, we[b])
        elif b >= 0:
            assert we[b] == tasks["w"][b], (name, we[b])
    for zdrop, band in ((7, 0), (6, 100), (0, 0)):  # condition 5: pen_total + o + e = 7 for the perfect flank
        pz = kswlib.make_params(zdrop=zdrop)
        a = idx["perfect"][0]
        assert extband_ref.w_eff(pz, pool, tasks[a:a + 1])[0] == band, zdrop
    for pz in (p, kswlib.make_params(zdrop=7), kswlib.make_params(zdrop=6)):
        narrow = tasks.copy()
        narrow["w"] = extband_ref.w_eff(pz, pool, tasks)
        full, _ = kswlib.orc_extend_batch(pz, pool, tasks)
        cut, _ = kswlib.orc_extend_batch(pz, pool, narrow)
        assert (full == cut).all()


def test_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, exe, plain = _build(tmp_path, "xb_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "xb_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, ["exhaustive", 4, 5])
    _run(exe, ["random", 20000, 5])
    small = tmp_path / "small.bin"
    tpool, ttasks = _targeted()
    with open(small, "wb") as f:
        f.write(struct.pack("<i", len(SCORINGS)))
        for kw in SCORINGS.values():
            _write_case(f, kswlib.make_params(**kw), 0, tpool, ttasks)
    _run(exe, ["file", small], list(SCORINGS))
