"""Mate rescue over a region table, the C-ABI without a GPU: bmh_matesw_table_device and bmh_last_matesw_table_stats are declared and
exported, the Python wrappers exist, the statistics record is 64 bytes with the fields where the wrapper reads them, and a call
without a context is refused before a device is touched."""
import ctypes as C
import os
import shutil
import subprocess

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
	S(bmh_matesw_table_stats_t); O(bmh_matesw_table_stats_t, regions_in); O(bmh_matesw_table_stats_t, regions_out);
	O(bmh_matesw_table_stats_t, arena_records); O(bmh_matesw_table_stats_t, hits); O(bmh_matesw_table_stats_t, mid_bytes);
	O(bmh_matesw_table_stats_t, pairs); O(bmh_matesw_table_stats_t, active); O(bmh_matesw_table_stats_t, waits);
	O(bmh_matesw_table_stats_t, filter_ms); O(bmh_matesw_table_stats_t, pack_ms); O(bmh_matesw_table_stats_t, merge_ms);
	S(bmh_alnreg_t); S(bmh_read_t); S(bmh_matesw_opt_t); S(bmh_pestat_t);
	return 0;
}
"""


def test_symbols_declarations_and_wrappers():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    assert "int bmh_matesw_table_device(bmh_ctx_t *ctx, int64_t l_pac, int n_pairs, const bmh_read_t *reads," in hdr
    assert "const uint64_t *roff, const bmh_alnreg_t *reg," in hdr
    assert "uint64_t *roff_out, bmh_alnreg_t **reg_out, int *n_sw);" in hdr
    assert "int bmh_last_matesw_table_stats(const bmh_ctx_t *ctx, bmh_matesw_table_stats_t *st);" in hdr
    assert hasattr(lib, "bmh_matesw_table_device") and hasattr(lib, "bmh_last_matesw_table_stats")
    assert callable(pkg.Context.matesw_table_device) and callable(pkg.Context.last_matesw_table_stats)
    assert pkg.MATESW_TABLE_STATS.itemsize == 64


def test_a_call_without_a_context_is_refused():
    pkg = load_package()
    lib = pkg.lib()
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    o = np.zeros((), dtype=kswlib.MATESW_OPT)
    roff = np.zeros(1, dtype=np.uint64)
    roff_out = np.full(1, 7, dtype=np.uint64)
    reg_out = C.c_void_p(None)
    args = (roff.ctypes.data_as(C.c_void_p), None, pes.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), C.c_float(0.95),
            roff_out.ctypes.data_as(C.c_void_p), C.cast(C.byref(reg_out), C.c_void_p), None)
    assert lib.bmh_matesw_table_device(None, C.c_int64(1000), 0, None, *args) == pkg.BMH_E_ARG
    assert roff_out[0] == 7 and reg_out.value is None
    st = np.zeros(1, dtype=pkg.MATESW_TABLE_STATS)
    assert lib.bmh_last_matesw_table_stats(None, st.ctypes.data_as(C.c_void_p)) == pkg.BMH_E_ARG


def test_stats_record_is_64_bytes(tmp_path):
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
    want = {"bmh_matesw_table_stats_t": 64, "bmh_alnreg_t": 64, "bmh_read_t": 16, "bmh_matesw_opt_t": 16, "bmh_pestat_t": 32}
    for name in pkg.MATESW_TABLE_STATS.names:
        want["bmh_matesw_table_stats_t." + name] = pkg.MATESW_TABLE_STATS.fields[name][1]
    assert got == want
