"""The C-ABI of bmh_reads_sam_device without a GPU: the call and bmh_last_reads_sam_stats are declared and exported, the hooks between
the library's translation units are not, bmh_reads_sam_stats_t keeps its 64-byte layout, and a NULL context or argument and a
paired-end flag are refused before a device is touched.  (With a context: tests/test_reads_sam_device_gpu.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

FIELDS = ("reads", "regions_in", "regions", "kmax", "opool_cap", "handoff_d2h_bytes", "waits_tail", "plan_ms", "neg_index")
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 52, 56]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(f) printf("." #f " %zu\n", offsetof(bmh_reads_sam_stats_t, f))
int main(void)
{
	S(bmh_reads_sam_stats_t); O(reads); O(regions_in); O(regions); O(kmax); O(opool_cap); O(handoff_d2h_bytes); O(waits_tail); O(plan_ms);
	O(neg_index); O(rsv_);
	printf("BMH_MEM_F_NO_EXACT %d\n", BMH_MEM_F_NO_EXACT);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("int bmh_reads_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o, "
            "const bmh_refidx_t *bns, const uint8_t *pac, int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text, "
            "int64_t *text_off);") in hdr
    assert "int bmh_last_reads_sam_stats(const bmh_ctx_t *ctx, bmh_reads_sam_stats_t *st);" in hdr
    for name in ("bmh_reads_sam_device", "bmh_last_reads_sam_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    assert not hasattr(lib, "bmh_samtext_check_reads_") and not hasattr(lib, "bmh_samtext_check_seqs_")
    for name in ("reads_sam_device", "last_reads_sam_stats"):
        assert callable(getattr(pkg.Context, name)), name


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
    want = {"bmh_reads_sam_stats_t": 64, ".rsv_": 60, "BMH_MEM_F_NO_EXACT": pkg.MEM_F_NO_EXACT}
    for name in FIELDS:
        want["." + name] = pkg.READS_SAM_STATS.fields[name][1]
    assert got == want
    assert pkg.READS_SAM_STATS.itemsize == 64 and pkg.READS_SAM_STATS.names == FIELDS + ("rsv",)
    assert [pkg.READS_SAM_STATS.fields[k][1] for k in FIELDS] == OFFSETS and pkg.MEM_F_NO_EXACT == 0x40


def test_refusals_without_a_context():
    """a NULL context with everything else in order, then each NULL argument: BMH_E_ARG, *text and text_off as they were"""
    pkg = load_package()
    lib = pkg.lib()
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    so, co = np.zeros(1, dtype=pkg.SMEM_OPT), np.zeros(1, dtype=pkg.CHAIN_OPT)
    idx = pkg.make_refidx([(0, 100)], 100, [b"chr"])
    pac = np.zeros(25, dtype=np.uint8)
    text = C.c_void_p(0x5a5a5a5a)
    off = np.full(2, -77, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = [None, p(so), p(co), 19, p(o), C.cast(C.byref(idx), C.c_void_p), p(pac), C.c_int64(0), 0, None, b"", C.cast(C.byref(text), C.c_void_p), p(off)]
    assert lib.bmh_reads_sam_device(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all()
    st = np.full(1, 7, dtype=pkg.READS_SAM_STATS)
    assert lib.bmh_last_reads_sam_stats(None, p(st)) == pkg.BMH_E_ARG and (st["reads"] == 7).all()


def test_stats_before_the_first_call():
    """every field -1 on a fresh context; without a device the context is refused loudly, which is all there is to see"""
    pkg = load_package()
    try:
        c = pkg.Context(0, kswlib.make_params())
    except pkg.BmhError as e:
        assert e.code == pkg.BMH_E_NODEVICE
        return
    try:
        st = c.last_reads_sam_stats()
        assert tuple(st) == FIELDS and all(v == -1 for v in st.values()), st
    finally:
        c.close()
