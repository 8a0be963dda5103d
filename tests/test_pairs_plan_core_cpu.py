"""The paired-end clause of host/handoff_core.h on the CPU: what table_plan_kernel folds over the region table mate rescue leaves on the
device (bmh_pairs_sam_device), as tests/pairs_plan_core_main.c runs it -- per slice of reads, the slices merged in three orders --
against a plain Python restatement of the loop in csrc/api.hip's decide_table_sizes.  Plainly, and under AddressSanitizer with the
offsets in a heap block of their exact size: vectors of 0 regions, one mate empty, a pair of 1024 and of 1025 regions (the edge of
BMH_HO_TAB_MAX), an odd trailing read, slices that cut pairs apart."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kswlib

SRC = os.path.join(kswlib.ROOT, "tests", "pairs_plan_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
TAB_MAX = 1 << 20
SLICES = (1, 2, 3, 64, 1000)


def pair_kmax(counts):
    """decide_table_sizes' loop over the vectors' lengths with BMH_MEM_F_PE: at every odd i, the pair (i - 1, i)"""
    k = 0
    for i in range(len(counts)):
        if i & 1:
            m = int(counts[i - 1]) + int(counts[i])
            k = max(k, TAB_MAX if m > 1024 else m * m + 1)
    return k


def _cases():
    rng = np.random.default_rng(5150)
    rnd = rng.integers(0, 40, 1000)
    rnd[rng.integers(0, 1000, 300)] = 0
    edge = lambda a, b: [3, 4, a, b, 0, 1]  # noqa: E731
    return [("no_reads", []), ("one_read", [7]), ("one_pair", [2, 3]), ("all_empty", [0] * 130), ("first_mate_empty", [0, 5, 1, 1]),
            ("second_mate_empty", [1, 1, 6, 0]), ("sum_1024", edge(1000, 24)), ("sum_1025", edge(1000, 25)), ("sum_1024_one_mate", edge(0, 1024)),
            ("sum_1025_one_mate", edge(1025, 0)), ("odd_trailing", [1, 1, 2, 2, 500]), ("odd_trailing_after_65", [1] * 64 + [30]),
            ("the_peak_in_the_last_pair", [1] * 128 + [9, 9]), ("the_peak_across_a_slice_edge", [1] * 2 + [20, 20] + [1] * 126), ("random_1000", rnd.tolist()),
            ("random_999", rnd[:999].tolist())]


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe)], capture_output=True, text=True)
    return gcc, exe, cc


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs_plan_cases")
    out = []
    for name, counts in _cases():
        path = d / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(np.array([0x50414952, len(counts)], dtype="<i4").tobytes())
            f.write(np.array(counts, dtype="<i8").tobytes())
        out.append((name, path, counts, pair_kmax(counts)))
    return out


def _check(exe, cases):
    for name, path, counts, want in cases:
        for slice_ in SLICES:
            run = subprocess.run([str(exe), str(path), str(slice_)], capture_output=True, text=True)
            assert run.returncode == 0, f"{name}, slices of {slice_}: exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
            m = re.fullmatch(r"reads (\d+) pairs (\d+) pair_kmax (\d+)\s*", run.stdout)
            assert m, run.stdout
            assert tuple(int(x) for x in m.groups()) == (len(counts), len(counts) // 2, want), (name, slice_, run.stdout, want)


def test_the_inputs_hold_every_clause(cases):
    by = {name: want for name, _, _, want in cases}
    assert by["no_reads"] == 0 and by["one_read"] == 0  # no pair: the clause adds nothing
    assert by["all_empty"] == 1 and by["one_pair"] == 26
    assert by["first_mate_empty"] == 26 and by["second_mate_empty"] == 37
    assert by["sum_1024"] == by["sum_1024_one_mate"] == 1024 * 1024 + 1 and by["sum_1025"] == by["sum_1025_one_mate"] == TAB_MAX
    assert by["sum_1024"] > by["sum_1025"]  # (both are out of a table of 2^20 entries: what counts is that neither overflows)
    assert by["odd_trailing"] == 17 and by["odd_trailing_after_65"] == 5  # the 500 and the 30 belong to no pair
    assert by["the_peak_in_the_last_pair"] == 325 and by["the_peak_across_a_slice_edge"] == 1601


def test_core_program_matches_the_restatement(cases, tmp_path):
    _, exe, cc = _build(tmp_path, "pp_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    assert cc.stderr.strip() == "", cc.stderr  # -Wall clean
    _check(exe, cases)


def test_core_program_under_sanitizer_with_an_exact_block(cases, tmp_path):
    gcc, _, plain = _build(tmp_path, "pp_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "pp_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _check(exe, cases)

