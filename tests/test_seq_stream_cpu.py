"""host/seqstream_core.h -- where the lane kernels' stream refill reads a sequence and how it assembles a dword of bases -- as a
stand-alone program (tests/seqstream_core_main.c), built plainly and under AddressSanitizer + UBSan.  The program compares every dword
with a byte-by-byte restatement and refuses a load outside the sequence; the sanitizer build adds the heap's own bounds."""
import os
import shutil
import subprocess

import pytest

import kswlib

SRC = os.path.join(kswlib.ROOT, "tests", "seqstream_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
# len 0..200 x 16 alignments x forward / reversed x (360 positions + 4 r0 x 17 shifts x 16 dwords)
N_DWORDS = 201 * 16 * 2 * (360 + 4 * 17 * 16)


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", "-Werror", *flags, SRC, "-o", str(exe)], capture_output=True, text=True)
    return gcc, exe, cc


def _run(exe):
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stderr[-4000:]}"
    assert run.stderr == ""
    word, n, loads = run.stdout.split()
    assert word == "ok" and int(n) == N_DWORDS
    # one load per dword of a sequence of four bases and more, three of one shorter, none of an empty one
    per_len = 16 * 2 * (360 + 4 * 17 * 16)
    assert int(loads) == per_len * (197 + 3 * 3)


def test_the_header_is_the_restatement(tmp_path):
    _, exe, cc = _build(tmp_path, "seqs_plain", [])
    assert cc.returncode == 0, cc.stderr
    _run(exe)


def test_the_header_under_sanitizers(tmp_path):
    gcc, _, plain = _build(tmp_path, "seqs_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "seqs_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _run(exe)
