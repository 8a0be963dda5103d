"""The mate-rescue device driver's C-ABI without a GPU: bmh_matesw_device is declared and exported, the records it shares with
bmh_matesw_batch keep their layouts, bad arguments are refused before a device is touched, and the preload shim refuses
BMH_MATESW_DEVICE=1 without a resident reference when it is loaded."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
	S(bmh_alnreg_t); O(bmh_alnreg_t, rb); O(bmh_alnreg_t, re); O(bmh_alnreg_t, qb); O(bmh_alnreg_t, qe); O(bmh_alnreg_t, score);
	O(bmh_alnreg_t, csub); O(bmh_alnreg_t, seedcov); O(bmh_alnreg_t, secondary);
	S(bmh_alnreg_v); S(bmh_read_t); S(bmh_sw_task_t); S(bmh_sw_result_t); S(bmh_matesw_opt_t); S(bmh_driver_stats_t);
	S(bmh_pestat_t); O(bmh_pestat_t, low); O(bmh_pestat_t, high); O(bmh_pestat_t, failed); O(bmh_pestat_t, avg); O(bmh_pestat_t, std);
	return 0;
}
"""


def test_symbol_wrapper_and_argument_checks():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    assert "int bmh_matesw_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads, bmh_alnreg_v *regs," in hdr
    assert "const bmh_pestat_t pes[4], const bmh_matesw_opt_t *o, float mask_level_redun, int *n_sw);" in hdr
    assert hasattr(lib, "bmh_matesw_device") and hasattr(lib, "bmh_matesw_batch")
    assert callable(pkg.Context.matesw_device) and callable(pkg.Context.matesw_batch)
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    o = np.zeros((), dtype=kswlib.MATESW_OPT)
    # no context: BMH_E_ARG, nothing else happens
    assert lib.bmh_matesw_device(None, C.c_int64(1000), 0, None, None, pes.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p),
                                 C.c_float(0.95), None) == pkg.BMH_E_ARG
    assert lib.bmh_matesw_device(None, C.c_int64(0), -1, None, None, None, None, C.c_float(0.95), None) == pkg.BMH_E_ARG


def test_record_layouts_are_unchanged(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    pkg = load_package()
    src = tmp_path / "layout.c"
    src.write_text(PROBE)
    cc = subprocess.run([gcc, "-I" + os.path.dirname(pkg.HEADER_PATH), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {"bmh_alnreg_t": 64, "bmh_alnreg_v": 24, "bmh_read_t": 16, "bmh_sw_task_t": 32, "bmh_sw_result_t": 32, "bmh_matesw_opt_t": 16,
            "bmh_driver_stats_t": 56, "bmh_pestat_t": 32}
    for name, off in zip(("low", "high", "failed", "avg", "std"), (kswlib.PESTAT.fields[k][1] for k in ("low", "high", "failed", "avg", "std"))):
        want["bmh_pestat_t." + name] = off
    for name in ("rb", "re", "qb", "qe", "score", "csub", "seedcov", "secondary"):
        want["bmh_alnreg_t." + name] = kswlib.ALNREG.fields[name][1]
    assert got == want
    assert kswlib.ALNREG.itemsize == 64 and kswlib.PESTAT.itemsize == 32 and kswlib.SW_TASK.itemsize == 32 and kswlib.SW_RES.itemsize == 32


def test_shim_refuses_matesw_device_without_resident_reference_at_load():
    """BMH_MATESW_DEVICE=1 with BMH_PAC_RESIDENT=0: status 1 when the shim is loaded, before any GPU work; it does not need
    BMH_REGS_DEVICE.  Loaded into a child interpreter behind the reference library."""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    code = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"
    env = {k: v for k, v in os.environ.items() if k not in ("BMH_REGS_DEVICE", "BMH_DEDUP_DEVICE")}
    env.update(BMH_MATESW_DEVICE="1", BMH_PAC_RESIDENT="0")
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert b"BMH_MATESW_DEVICE=1 needs the reference resident" in r.stderr and b"loaded" not in r.stdout
    env["BMH_PAC_RESIDENT"] = "1"
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"loaded" in r.stdout, r.stderr.decode()[-500:]
