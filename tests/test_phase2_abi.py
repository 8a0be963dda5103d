"""The C-ABI of the fused phase 2 call without a GPU: bmh_phase2_device, its switch and bmh_last_phase2_stats are declared and
exported, bmh_phase2_stats_t keeps its 72-byte layout, and a NULL context is refused before a device is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

FIELDS = ("units", "wanted", "fixed", "redone", "fallbacks", "h2d_bytes", "d2h_bytes", "waits", "sessions", "decide_ms", "wanted_ms")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
	S(bmh_phase2_stats_t); O(bmh_phase2_stats_t, units); O(bmh_phase2_stats_t, wanted); O(bmh_phase2_stats_t, fixed); O(bmh_phase2_stats_t, redone);
	O(bmh_phase2_stats_t, fallbacks); O(bmh_phase2_stats_t, h2d_bytes); O(bmh_phase2_stats_t, d2h_bytes); O(bmh_phase2_stats_t, waits);
	O(bmh_phase2_stats_t, sessions); O(bmh_phase2_stats_t, decide_ms); O(bmh_phase2_stats_t, wanted_ms);
	S(bmh_wanted_res_t); S(bmh_pairdec_t);
	printf("BMH_VERSION %d\n", BMH_VERSION);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("int bmh_phase2_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, "
            "int64_t id0, int n, const bmh_read_t *reads, bmh_alnreg_v *regs, const int64_t *roff, bmh_pairdec_t *pd, int32_t *reg_mapq, "
            "int32_t *n_want, int32_t *want_k, bmh_wanted_res_t *results, int64_t results_cap, int64_t *n_wanted, uint32_t *cigar_pool, "
            "size_t cigar_words, char *md_pool, size_t md_bytes);") in hdr
    assert "int bmh_ctx_set_phase2_device(bmh_ctx_t *ctx, int on);" in hdr
    assert "int bmh_last_phase2_stats(const bmh_ctx_t *ctx, bmh_phase2_stats_t *st);" in hdr
    assert ("typedef struct bmh_phase2_stats { int64_t units, wanted, fixed, redone, fallbacks; int64_t h2d_bytes, d2h_bytes; int32_t waits, sessions; "
            "float decide_ms, wanted_ms; } bmh_phase2_stats_t;") in hdr
    for name in ("bmh_phase2_device", "bmh_ctx_set_phase2_device", "bmh_last_phase2_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    # the hook between the library's own translation units is not part of the interface
    assert not hasattr(lib, "bmh_phase2_routed_")
    for name in ("phase2_device", "set_phase2_device", "last_phase2_stats"):
        assert callable(getattr(pkg.Context, name)), name
    assert lib.bmh_version() == 310


def test_stats_layout(tmp_path):
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
    want = {"bmh_phase2_stats_t": 72, "bmh_wanted_res_t": 72, "bmh_pairdec_t": 48, "BMH_VERSION": 310}
    for name in FIELDS:
        want["bmh_phase2_stats_t." + name] = pkg.PHASE2_STATS.fields[name][1]
    assert got == want
    assert pkg.PHASE2_STATS.itemsize == 72 and pkg.PHASE2_STATS.names == FIELDS
    assert [pkg.PHASE2_STATS.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68]


def test_refusals_without_a_context():
    pkg = load_package()
    lib = pkg.lib()
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    n_wanted = C.c_int64(7)
    st = np.full(1, 7, dtype=pkg.PHASE2_STATS)
    rc = lib.bmh_phase2_device(None, o.ctypes.data_as(C.c_void_p), None, None, None, C.c_int64(0), 0, None, None, None, None, None, None, None, None,
                               C.c_int64(0), C.cast(C.byref(n_wanted), C.c_void_p), None, C.c_size_t(0), None, C.c_size_t(0))
    assert rc == pkg.BMH_E_ARG and n_wanted.value == 7
    assert lib.bmh_ctx_set_phase2_device(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_phase2_stats(None, st.ctypes.data_as(C.c_void_p)) == pkg.BMH_E_ARG
    assert (st["units"] == 7).all()


def test_stats_before_the_first_call():
    """every field -1 on a fresh context; without a device the context is refused loudly, which is all there is to see"""
    pkg = load_package()
    try:
        c = pkg.Context(0, kswlib.make_params())
    except pkg.BmhError as e:
        assert e.code == pkg.BMH_E_NODEVICE
        return
    try:
        st = c.last_phase2_stats()
        assert tuple(st) == FIELDS and all(v == -1 for v in st.values()), st
        c.set_phase2_device(True), c.set_phase2_device(False)
        assert all(v == -1 for v in c.last_phase2_stats().values())
    finally:
        c.close()
