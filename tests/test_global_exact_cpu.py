"""The global dispatcher's bin and sort-key rule (host/glbbin_core.h) against its restatement in Python (glbbin_ref.py), which
tests/test_global_exact_gpu.py uses to predict bmh_last_global_bin_counts; the header as a stand-alone program
(tests/glbbin_core_main.c), built plainly and under AddressSanitizer + UBSan; and the rule on the bands of the bench's own generator:
enough of its tasks must fall into the exact-band bins 6 and 7 for the GPU test to mean anything."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import glbband_ref
import glbbin_ref as br
import kswlib
from __graft_entry__ import load_package

SRC = os.path.join(kswlib.ROOT, "tests", "glbbin_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", "-Werror", *flags, SRC, "-o", str(exe)], capture_output=True, text=True)
    return gcc, exe, cc


def _run_and_compare(exe):
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stderr[-4000:]}"
    rows = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == 301 * 2 * 3 * 19
    for w, c32, exact, tlen, b, key in rows:
        assert b == br.lane_bin(w, c32, exact), (w, c32, exact, b)
        assert key == br.sort_key(b, tlen, w), (w, c32, exact, tlen, b, key)
    return rows


def test_the_header_is_the_restatement(tmp_path):
    _, exe, cc = _build(tmp_path, "gbin_plain", [])
    assert cc.returncode == 0, cc.stderr
    rows = _run_and_compare(exe)
    assert {r[4] for r in rows} == {0, 1, 2, 3, 5, 6, 7}
    # both sides of 3/4 and 7/8 at every level of the switch
    assert [br.lane_bin(w, 1, 7) for w in (0, 3, 4, 7, 8, 15, 16)] == [6, 6, 7, 7, 5, 5, 0]
    assert [br.lane_bin(w, 1, 3) for w in (0, 3, 4, 7, 8)] == [6, 6, 5, 5, 5]
    assert [br.lane_bin(w, 1, 0) for w in (0, 3, 4, 7, 8)] == [5, 5, 5, 5, 5]
    assert [br.lane_bin(w, 0, 7) for w in (3, 4, 7, 8)] == [6, 7, 7, 0]


def test_the_header_under_sanitizers(tmp_path):
    gcc, _, plain = _build(tmp_path, "gbin_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "gbin_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run_and_compare(exe)


@pytest.fixture(scope="module")
def bench_tasks():
    tg = importlib.import_module(load_package().__name__ + ".taskgen")
    pool, tasks, _ = tg.generate_global(20000, "150bp", seed=939)
    assert len(tasks) == 20000
    return pool, tasks


def test_the_generators_bands_fill_the_exact_bins(bench_tasks):
    pool, tasks = bench_tasks
    p = kswlib.make_params()
    bins, ws = br.expected_bins(p, pool, tasks)
    bands = glbband_ref.expected_bands(p, pool, tasks)
    n = len(tasks)
    share = {b: float((bins == b).sum()) / n for b in range(8)}
    print("share of tasks per bin:", {b: round(s, 4) for b, s in share.items()})
    print("share per band 0..7:", [round(float((bands == w).sum()) / n, 4) for w in range(8)])
    assert (ws[bins != 2] == bands[bins != 2]).all()
    assert ((bins == 6) == (bands <= 3)).all() and ((bins == 7) == ((bands >= 4) & (bands <= 7))).all()  # every task of this shape is in the lane domain
    # the reference rule alone gives 53.8 % and 28.5 %
    assert share[6] >= 0.45 and share[7] >= 0.20, share
    assert (br.expected_counts(p, pool, tasks) == np.bincount(bins, minlength=8)).all()
    # level 3 moves bin 7's tasks back to the 32-slot kernel, level 0 both
    c3, c0 = br.expected_counts(p, pool, tasks, exact=3), br.expected_counts(p, pool, tasks, exact=0)
    c7 = br.expected_counts(p, pool, tasks)
    assert c3[6] == c7[6] and c3[7] == 0 and c3[5] == c7[5] + c7[7] and c0[6] == c0[7] == 0 and c0[5] == c7[5] + c7[6] + c7[7]
    # without the band pass the tasks' own w (|delta| + 3 + U[0, 32]) picks the bins
    own = br.expected_bins(p, pool, tasks, narrow=False)
    assert (own[1] == tasks["w"]).all() and 0 < (own[0] == 6).sum() < (bins == 6).sum()


def test_band_major_order_keeps_waves_uniform(bench_tasks):
    pool, tasks = bench_tasks
    p = kswlib.make_params()
    bins, ws = br.expected_bins(p, pool, tasks)
    for b, lo in ((6, 0), (7, 4)):
        waves = br.narrow_waves(bins, ws, tasks["tlen"], b)
        assert sum(len(x) for x in waves) >= len(waves) and all(lo <= w <= lo + 3 for x in waves for w in x)
        firsts = [x[-1] for x in waves]  # widest band first, never back to a wider one
        assert firsts == sorted(firsts, reverse=True)
        seams = br.seam_waves(bins, ws, tasks["tlen"], b)
        print(f"bin {b}: {len(waves)} waves, {seams} with more than one band")
        assert seams <= 3  # four bands meet at three places at the most
