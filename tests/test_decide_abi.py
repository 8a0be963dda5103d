"""The C-ABI of pass A of phase 2 without a GPU: bmh_decide_batch, bmh_decide_device, the context switch and its statistics are
declared and exported, bmh_pairdec_t keeps its 48-byte layout, and bad arguments are refused before a device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
	S(bmh_pairdec_t); O(bmh_pairdec_t, paired); O(bmh_pairdec_t, z); O(bmh_pairdec_t, q_se); O(bmh_pairdec_t, extra_flag); O(bmh_pairdec_t, score);
	O(bmh_pairdec_t, sub); O(bmh_pairdec_t, n_sub); O(bmh_pairdec_t, q_pe); O(bmh_pairdec_t, rsv);
	S(bmh_sam_opt_t); S(bmh_pestat_t); S(bmh_alnreg_t); S(bmh_alnreg_v);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("typedef struct bmh_pairdec { int32_t paired, z[2], q_se[2], extra_flag, score, sub, n_sub, q_pe, rsv[2]; } bmh_pairdec_t;") in hdr
    args = ("const bmh_sam_opt_t *o, int64_t l_pac, const bmh_pestat_t *pes, int64_t id0, int n, bmh_alnreg_v *regs, const int64_t *roff, "
            "bmh_pairdec_t *pd, int32_t *reg_mapq, int32_t *n_want, int32_t *want_k);")
    assert "int bmh_decide_batch(" + args in hdr
    assert "int bmh_decide_device(bmh_ctx_t *ctx, " + args in hdr
    assert "int bmh_ctx_set_decide_device(bmh_ctx_t *ctx, int on);" in hdr
    assert "int bmh_last_decide_stats(const bmh_ctx_t *ctx, int64_t *units, int64_t *fallbacks, float *kernel_ms);" in hdr
    for name in ("bmh_decide_batch", "bmh_decide_device", "bmh_ctx_set_decide_device", "bmh_last_decide_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    # helpers between the library's own translation units are not part of the interface
    for name in ("bmh_decide_routed_", "bmh_decide_stats_reset_", "bmh_pp_fill_log_", "bmh_pp_fill_term_"):
        assert not hasattr(lib, name), name
    assert callable(pkg.decide_batch) and callable(pkg.Context.decide_device) and callable(pkg.Context.set_decide_device)
    assert callable(pkg.Context.last_decide_stats)


def test_pairdec_layout(tmp_path):
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
    want = {"bmh_pairdec_t": 48, "bmh_sam_opt_t": 96, "bmh_pestat_t": 32, "bmh_alnreg_t": 64, "bmh_alnreg_v": 24}
    for name in ("paired", "z", "q_se", "extra_flag", "score", "sub", "n_sub", "q_pe", "rsv"):
        want["bmh_pairdec_t." + name] = pkg.PAIRDEC.fields[name][1]
    assert got == want
    assert pkg.PAIRDEC.itemsize == 48 and pkg.SAM_OPT.itemsize == 96
    assert [pkg.PAIRDEC.fields[k][1] for k in ("paired", "z", "q_se", "extra_flag", "score", "sub", "n_sub", "q_pe", "rsv")] == [0, 4, 12, 20, 24, 28, 32, 36, 40]


def test_refusals_without_a_context():
    pkg = load_package()
    lib = pkg.lib()
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    p = o.ctypes.data_as(C.c_void_p)
    assert lib.bmh_decide_device(None, p, C.c_int64(1000), None, C.c_int64(0), 0, None, None, None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_decide_device(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_decide_stats(None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_decide_batch(None, C.c_int64(1000), None, C.c_int64(0), 0, None, None, None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_decide_batch(p, C.c_int64(1000), None, C.c_int64(0), -1, None, None, None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_decide_batch(p, C.c_int64(1000), None, C.c_int64(0), 3, None, None, None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_decide_batch(p, C.c_int64(1000), None, C.c_int64(0), 0, None, None, None, None, None, None) == pkg.BMH_OK
