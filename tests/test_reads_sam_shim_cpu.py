"""The preload shim's single-end session (BMH_READS_SAM_DEVICE=1) without a GPU: the refusal when the library is loaded, the pipeline
tool's flag, the helper that cuts a batch's text into the reads' strings (host/samcut_core.h: no symbol of either library, the one text
of both callers, and as a program of its own plainly and under AddressSanitizer), and the version, which the switch does not move."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import kswlib
from __graft_entry__ import load_package

SRC = os.path.join(kswlib.ROOT, "tests", "samcut_core_main.c")
HOST = os.path.join(kswlib.ROOT, "bwa-mem-quickassist_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
MESSAGE = b"[bwamem_hip] fatal: BMH_READS_SAM_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n"
# (reads, seed, the allocation that fails or -1) -> the return code; -5 is BMH_E_NOMEM
RUNS = [((0, 1, -1), 0), ((1, 2, -1), 0), ((4, 3, -1), 0), ((1000, 4, -1), 0), ((1000, 5, 0), -5), ((1000, 6, 499), -5), ((1000, 7, 999), -5), ((1, 8, 0), -5)]


def test_shim_refuses_the_switch_without_resident_reference_at_load():
    """BMH_READS_SAM_DEVICE=1 with BMH_PAC_RESIDENT=0: the shim says so and leaves with status 1 when it is loaded, before any GPU work.
    Loaded into a child interpreter behind the reference library, as test_region_long_abi.py loads it."""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    code = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"
    env = dict(os.environ, BMH_READS_SAM_DEVICE="1", BMH_PAC_RESIDENT="0")
    for k in ("BMH_REGS_DEVICE", "BMH_MATESW_DEVICE", "BMH_WANTED_DEVICE", "BMH_PHASE2_DEVICE", "BMH_PHASE2_TEXT_DEVICE", "BMH_REGION_LONG"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert MESSAGE in r.stderr and b"loaded" not in r.stdout
    env.pop("BMH_PAC_RESIDENT")
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"loaded" in r.stdout, r.stderr.decode()[-500:]


def test_pipeline_tool_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(kswlib.ROOT, "tools", "pipeline_bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--reads-sam-device" in r.stdout and "BMH_READS_SAM_DEVICE=1" in r.stdout


def test_the_cut_is_one_text_and_no_symbol_of_either_library():
    pkg = load_package()
    nm = shutil.which("nm")
    if not nm:
        pytest.skip("no nm")
    for lib in (pkg.LIB_PATH, pkg.DROPIN_PATH):
        assert os.path.exists(lib), lib
        syms = subprocess.run([nm, "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert "bmh_sam_batch" in syms or "mem_process_seqs" in syms  # (the listing is the library's)
        assert "bmh_sam_cut" not in syms, lib
    # both callers go through it, and neither keeps a loop of its own
    post = open(os.path.join(HOST, "sam_post.c")).read()
    shim = open(os.path.join(HOST, "interpose.c")).read()
    assert '#include "samcut_core.h"' in post and '#include "samcut_core.h"' in shim
    assert post.count("bmh_sam_cut(") == 1 and shim.count("bmh_sam_cut(") == 1
    assert ".sam = s" not in post and ".sam = s" not in shim
    assert "static int bmh_sam_cut(" in open(os.path.join(HOST, "samcut_core.h")).read()


def test_version_is_what_the_header_says():
    pkg = load_package()
    m = re.search(r"#define BMH_VERSION (\d+)", open(pkg.HEADER_PATH).read())
    assert m and pkg.lib().bmh_version() == int(m.group(1)) == 310  # no exported symbol or record changed with the switch


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe)], capture_output=True, text=True)
    return gcc, exe, cc


def _check(exe):
    for (n, seed, fail_at), want in RUNS:
        run = subprocess.run([str(exe), str(n), str(seed), str(fail_at)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, f"{(n, seed, fail_at)}: exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
        m = re.fullmatch(r"reads (\d+) bytes (\d+) strings (\d+) rc (-?\d+)\s*", run.stdout)
        assert m, run.stdout
        got_n, nbytes, strings, rc = (int(x) for x in m.groups())
        assert (got_n, rc, strings) == (n, want, n if want == 0 else 0), (n, seed, fail_at, run.stdout)
        assert nbytes > 0 or n == 0


def test_cut_program_plainly(tmp_path):
    _, exe, cc = _build(tmp_path, "cut_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    assert cc.stderr.strip() == "", cc.stderr  # -Wall clean
    _check(exe)


def test_cut_program_under_sanitizer_with_exact_blocks(tmp_path):
    gcc, _, plain = _build(tmp_path, "cut_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "cut_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _check(exe)
