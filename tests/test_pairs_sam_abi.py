"""The C-ABI of bmh_pairs_sam_device without a GPU: the call and bmh_last_pairs_sam_stats are declared and exported,
bmh_pairs_sam_stats_t keeps its 128-byte layout, and a NULL context or argument, an odd n and a missing paired-end flag are refused
before a device is touched, with *text and text_off as they were.  (With a context: tests/test_pairs_sam_device_gpu.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

FIELDS = ("reads", "pairs", "regions_in", "regions", "regions_out", "n_sw", "kmax", "pair_kmax", "opool_cap", "mid_d2h_bytes", "mid_h2d_bytes",
          "waits_mid", "pes_given", "plan_ms", "neg_index")
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92, 96, 100]
MEM_F_PE = 0x2

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(f) printf("." #f " %zu\n", offsetof(bmh_pairs_sam_stats_t, f))
int main(void)
{
	S(bmh_pairs_sam_stats_t); O(reads); O(pairs); O(regions_in); O(regions); O(regions_out); O(n_sw); O(kmax); O(pair_kmax); O(opool_cap);
	O(mid_d2h_bytes); O(mid_h2d_bytes); O(waits_mid); O(pes_given); O(plan_ms); O(neg_index); O(rsv_);
	printf("BMH_MEM_F_PE %d\n", BMH_MEM_F_PE);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("int bmh_pairs_sam_device(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_matesw_opt_t *mo, "
            "const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes0, bmh_pestat_t pes_out[4] /* nullable */, "
            "int64_t id0, int n, const bmh_seq_t *seqs, const char *rg_id, char **text, int64_t *text_off);") in hdr
    assert "int bmh_last_pairs_sam_stats(const bmh_ctx_t *ctx, bmh_pairs_sam_stats_t *st);" in hdr
    for name in ("bmh_pairs_sam_device", "bmh_last_pairs_sam_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    for name in ("pairs_sam_device", "last_pairs_sam_stats"):
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
    want = {"bmh_pairs_sam_stats_t": 128, ".rsv_": 104, "BMH_MEM_F_PE": MEM_F_PE}
    for name in FIELDS:
        want["." + name] = pkg.PAIRS_SAM_STATS.fields[name][1]
    assert got == want
    assert pkg.PAIRS_SAM_STATS.itemsize == 128 and pkg.PAIRS_SAM_STATS.names == FIELDS + ("rsv",)
    assert [pkg.PAIRS_SAM_STATS.fields[k][1] for k in FIELDS] == OFFSETS


def _args(pkg, keep, flag=MEM_F_PE, n=0):
    """every argument in order for a call without a context; keep holds what the pointers point to"""
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    o["flag"] = flag
    so, co, mo = np.zeros(1, dtype=pkg.SMEM_OPT), np.zeros(1, dtype=pkg.CHAIN_OPT), np.zeros(1, dtype=pkg.MATESW_OPT)
    idx = pkg.make_refidx([(0, 100)], 100, [b"chr"])
    pac = np.zeros(25, dtype=np.uint8)
    text = C.c_void_p(0x5a5a5a5a)
    off = np.full(n + 2, -77, dtype=np.int64)
    pes, pes_out = np.zeros(4, dtype=pkg.PESTAT), np.full(4, 9, dtype=pkg.PESTAT)
    seqs = np.zeros(64 * max(n, 1), dtype=np.uint8)  # (never read: every refusal here comes before the reads are looked at)
    keep += [o, so, co, mo, idx, pac, text, off, pes, pes_out, seqs]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return [None, p(so), p(co), 19, p(mo), p(o), C.cast(C.byref(idx), C.c_void_p), p(pac), p(pes), p(pes_out), C.c_int64(0), n, p(seqs) if n else None, b"",
            C.cast(C.byref(text), C.c_void_p), p(off)], text, off, pes_out


def test_refusals_without_a_context():
    """a NULL context with everything else in order: BMH_E_ARG, *text, text_off and pes_out as they were"""
    pkg = load_package()
    lib = pkg.lib()
    keep = []
    args, text, off, pes_out = _args(pkg, keep)
    assert lib.bmh_pairs_sam_device(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all() and (pes_out["low"] == 9).all()
    for null in (1, 2, 4, 5, 6, 14, 15):  # so, co, mo, o, bns, text, text_off: no crash on the way to the answer
        args, text, off, pes_out = _args(pkg, keep)
        args[null] = None
        assert lib.bmh_pairs_sam_device(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all(), null
    for flag, n in ((MEM_F_PE, 1), (MEM_F_PE, 3), (0, 2)):  # an odd n, a missing BMH_MEM_F_PE: here the NULL context answers first (no crash, no write)
        args, text, off, pes_out = _args(pkg, keep, flag=flag, n=n)
        assert lib.bmh_pairs_sam_device(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all() and (pes_out["low"] == 9).all(), (flag, n)
    st = np.full(1, 7, dtype=pkg.PAIRS_SAM_STATS)
    assert lib.bmh_last_pairs_sam_stats(None, st.ctypes.data_as(C.c_void_p)) == pkg.BMH_E_ARG and (st["reads"] == 7).all()


def _context(pkg):
    """a context, or a skip that says why: what follows the NULL-context test needs one, and a context needs a device"""
    try:
        return pkg.Context(0, kswlib.make_params())
    except pkg.BmhError as e:
        assert e.code == pkg.BMH_E_NODEVICE
        pytest.skip("no device: a context cannot be made, and without one every refusal is the NULL context's")


def test_refusals_of_the_arguments():
    """each NULL argument, an odd n and a missing BMH_MEM_F_PE, each answered by the check that names it: BMH_E_ARG before anything
    is touched, the sentinels intact.  Needs a context to get past the first check of all, so it is skipped where there is no device"""
    pkg = load_package()
    lib = pkg.lib()
    c = _context(pkg)
    try:
        h = c._h
        for null in (1, 2, 4, 5, 6, 14, 15):  # so, co, mo, o, bns, text, text_off
            keep = []
            args, text, off, pes_out = _args(pkg, keep)
            args[0], args[null] = h, None
            assert lib.bmh_pairs_sam_device(*args) == pkg.BMH_E_ARG, null
            assert text.value == 0x5a5a5a5a and (off == -77).all() and (pes_out["low"] == 9).all(), null
        for flag, n in ((MEM_F_PE, 1), (MEM_F_PE, 3), (0, 2), (0, 0)):
            keep = []
            args, text, off, pes_out = _args(pkg, keep, flag=flag, n=n)
            args[0] = h
            assert lib.bmh_pairs_sam_device(*args) == pkg.BMH_E_ARG, (flag, n)
            assert text.value == 0x5a5a5a5a and (off == -77).all() and (pes_out["low"] == 9).all(), (flag, n)
            why = lib.bmh_last_error(h).decode()
            assert ("odd" if flag else "BMH_MEM_F_PE") in why, why
    finally:
        c.close()


def test_stats_before_the_first_call():
    """every field -1 on a fresh context (skipped where no context can be made)"""
    pkg = load_package()
    c = _context(pkg)
    try:
        st = c.last_pairs_sam_stats()
        assert tuple(st) == FIELDS and all(v == -1 for v in st.values()), st
    finally:
        c.close()
