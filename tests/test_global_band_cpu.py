"""host/glbband_core.h -- the band a ksw_global2 task needs for its result -- as a stand-alone program
(tests/glbband_core_main.c) built once plainly and once under AddressSanitizer, every sequence in a heap block of exactly its length.
For every task: |qlen - tlen| <= w_eff <= w (w_eff == w where the rule does not apply), and the oracle's ksw_global2 at w_eff returns
the score, n_cigar and every CIGAR word it returns at w."""
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import glbband_ref
import kswgen
import kswlib
from __graft_entry__ import load_package

SRC = os.path.join(kswlib.ROOT, "tests", "glbband_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LINE = re.compile(r"case (\d+): (\d+) tasks, (\d+) applied, (\d+) narrowed, (\d+) range errors, (\d+) differ, cells (\d+) -> (\d+)")
WEFF = re.compile(r"weff (\d+):([ \d-]*)")

DEFAULT = dict()
SCORINGS = {"a2b8": dict(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2), "odel_ne_oins": dict(o_del=6, o_ins=4, e_del=1, e_ins=2),
            "e2": dict(e_del=2, e_ins=2), "open0": dict(o_del=0, o_ins=0)}


def _taskgen():
    return importlib.import_module(load_package().__name__ + ".taskgen")


def low_complexity(rng, n):
    """Repeats of period 1-4 with about 5 % errors and a phase shift between the read and its window."""
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for _ in range(n):
        unit = rng.integers(0, 4, size=int(rng.integers(1, 5)), dtype=np.uint8)
        L, phase = int(rng.integers(60, 151)), int(rng.integers(0, 5))
        q = np.tile(unit, L // len(unit) + 3)[:L]
        t = kswgen.mutate(rng, np.tile(unit, L // len(unit) + 4)[phase:phase + L], 0.04, 0.005, 0.005, 3)
        if len(t) == 0:
            t = kswgen.rand_seq(rng, 1)
        kswgen._add_glb(pb, q, t, abs(len(q) - len(t)) + 3 + int(rng.integers(0, 33)))
    return kswgen.finish_glb(pb)[:2]


def with_n(rng, n):
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for _ in range(n):
        q = kswgen.rand_seq(rng, int(rng.integers(40, 151)), 0.05)
        src = q.copy()
        src[src > 3] = 0
        t = kswgen.mutate(rng, src, 0.02, 0.004, 0.004, 4)
        t[rng.random(len(t)) < 0.03] = 4
        if len(t) == 0:
            t = kswgen.rand_seq(rng, 1)
        kswgen._add_glb(pb, q, t, abs(len(q) - len(t)) + int(rng.integers(0, 36)))
    return kswgen.finish_glb(pb)[:2]


def edge_tasks():
    """(pool, tasks, what each w_eff must be: an exact value, or ('ge', k))"""
    rng = np.random.default_rng(3)
    pb, want = kswgen.PoolBuilder(kswlib.GLB_TASK), []

    def add(q, t, w, expect):
        kswgen._add_glb(pb, np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8), w)
        want.append(expect)

    base = kswgen.rand_seq(rng, 100)

    def mism(k):
        t = base.copy()
        for p in (10, 40, 70, 90)[:k]:
            t[p] = (t[p] + 1) & 3
        return t

    add(base, base[:80], 10, 10)          # w < |delta|: left alone
    add(base[:80], base, 19, 19)          # ... and on the other side
    add(base, base[:80], 20, 20)          # w == |delta|
    add(base[:70], base, 30, 30)
    add(base[:1], base[:40], 50, ("ge", 39))  # qlen 1
    add(base[:40], base[:1], 50, ("ge", 39))  # tlen 1
    add(base[:1], base[:1], 7, 0)
    add(base[:1], [(int(base[0]) + 1) & 3], 7, 0)
    for k in (0, 1, 2):
        add(base, mism(k), 25, 0)         # equal lengths, k mismatches: the diagonal beats every path with two gaps
    add(base, mism(3), 25, ("ge", 1))     # three: UB(1) EQUALS the diagonal's score, and the rule is strict
    add(base, mism(4), 25, ("ge", 1))
    add(base, base, 0, 0)
    add(base, base[:0], 5, 5)             # an empty target: left alone
    add(base[:0], base, 5, 5)
    add(base, base, -1, -1)               # a negative w is below |delta| = 0: left alone
    pool, tasks, _ = kswgen.finish_glb(pb)
    return pool, tasks, want


def _write_case(f, p, mode, pool, tasks):
    p = np.ascontiguousarray(p, dtype=kswlib.PARAMS)
    tasks = np.ascontiguousarray(tasks, dtype=kswlib.GLB_TASK)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    f.write(p.tobytes() + struct.pack("<iq", mode, len(pool)) + pool.tobytes() + struct.pack("<i", len(tasks)) + tasks.tobytes())


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the input file, names of the cases in order, the edge cases' expectations)"""
    tg = _taskgen()
    rng = np.random.default_rng(20)
    g150 = tg.generate_global(3000, "150bp", seed=939, wspread=32)[:2]
    gmix = tg.generate_global(2000, "mixed100-300", seed=939, wspread=32)[:2]
    low, ns = low_complexity(rng, 2500), with_n(rng, 2000)
    epool, etasks, ewant = edge_tasks()
    big = tg.generate_global(200000, "150bp", seed=939)[:2]
    sets = [("150bp", DEFAULT, 1, g150), ("mixed100-300", DEFAULT, 1, gmix), ("low", DEFAULT, 1, low), ("N", DEFAULT, 1, ns),
            ("edges", DEFAULT, 3, (epool, etasks)), ("ratio", DEFAULT, 0, big)]
    for name, kw in SCORINGS.items():
        sets.append((name + "/150bp", kw, 1, (g150[0], g150[1][:1500])))
        sets.append((name + "/low", kw, 1, (low[0], low[1][:1500])))
        sets.append((name + "/edges", kw, 1, (epool, etasks)))
    # every pair of short sequences at every band, ties and zero costs included (glbband_ref.py): the sets the GPU test reads the bands of
    small = (("A", glbband_ref.set_a()[:2]), ("B", glbband_ref.set_b()[:2]))
    for name, kw in glbband_ref.SCORINGS.items():
        for s, pt in small:
            sets.append((f"small{s}/{name}", kw, 1, pt))
    # a matrix without a positive entry, and a negative gap cost: the rule must leave every w alone
    sets.append(("A<=0", dict(mat=np.minimum(kswlib.fill_scmat(1, 4), 0)), 0, (g150[0], g150[1][:300])))
    sets.append(("e<0", dict(e_del=-1), 0, (g150[0], g150[1][:300])))
    path = tmp_path_factory.mktemp("glbband") / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(sets)))
        for _, kw, mode, (pool, tasks) in sets:
            _write_case(f, kswlib.make_params(**kw), mode, pool, tasks)
    return path, [s[0] for s in sets], ewant


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    kswlib.load_oracle()  # liborc.so is there
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-L" + kswlib.ORACLE_DIR, "-lorc", "-Wl,-rpath," + kswlib.ORACLE_DIR],
                        capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe, cases):
    path, names, _ = cases
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    rows = [tuple(int(x) for x in m) for m in LINE.findall(run.stdout)]
    print("\n".join(f"{n}: {r}" for n, r in zip(names, rows)))  # every figure, before anything is asserted
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert len(rows) == len(names) and all(r[4] == 0 and r[5] == 0 for r in rows), rows
    weff = {int(c): [int(x) for x in v.split()] for c, v in WEFF.findall(run.stdout)}
    return dict(zip(names, rows)), weff


def test_narrow_band_gives_the_oracles_result_and_the_rule_bites(cases, tmp_path):
    _, exe, cc = _build(tmp_path, "gb_plain", [])
    assert cc.returncode == 0, cc.stderr
    rows, weff = _run(exe, cases)
    names, ewant = cases[1], cases[2]
    # the sets are not vacuous: most tasks are narrowed, so most were compared with the oracle
    for name in ("150bp", "low", "N", "a2b8/150bp", "odel_ne_oins/150bp", "e2/150bp", "open0/150bp"):
        _, n, applied, narrowed, _, _, c0, c1 = rows[name]
        assert applied == n and narrowed > n // 2 and c1 < c0, (name, rows[name])
    assert rows["mixed100-300"][3] > 200 and rows["low"][7] < rows["low"][6]
    for name in glbband_ref.SCORINGS:  # the exhaustive sets: whole, the rule applied to all, and a good part narrowed (so compared with the oracle)
        a, b = rows[f"smallA/{name}"], rows[f"smallB/{name}"]
        assert a[1] == a[2] == 22732 and b[1] == b[2] == 6741 and 7000 < a[3] < 18000 and 1500 < b[3] < 5000, (name, a, b)
    for name in ("A<=0", "e<0"):
        assert rows[name][2] == 0 and rows[name][3] == 0 and rows[name][6] == rows[name][7], (name, rows[name])
    # the edges, value by value
    got = weff[names.index("edges")]
    assert len(got) == len(ewant)
    for k, (g, e) in enumerate(zip(got, ewant)):
        assert (g >= e[1] if isinstance(e, tuple) else g == e), (k, g, e)
    # the rule has not decayed into a no-op: the bench's own task set, cells counted in the 8-slot blocks the lane kernels compute
    _, n, _, _, _, _, c0, c1 = rows["ratio"]
    print(f"ratio {c1 / c0:.4f}")
    assert n == 200000 and c1 / c0 < 0.45, (c0, c1)


def test_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, exe, plain = _build(tmp_path, "gb_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "gb_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe, cases)
