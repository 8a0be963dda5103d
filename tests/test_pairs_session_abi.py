"""The C-ABI of the paired-end session in two calls without a GPU: bmh_pairs_sam_begin, bmh_pairs_sam_finish, bmh_pairs_parked_free,
bmh_pairs_parked_info and bmh_pairs_parked_trim are declared and exported, bmh_pairs_parked_info_t keeps its 24-byte layout, NULL
arguments are refused before a device is touched with the caller's memory as it was, and freeing NULL does nothing.  (With a context:
tests/test_pairs_session_gpu.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package

SYMBOLS = ("bmh_pairs_sam_begin", "bmh_pairs_sam_finish", "bmh_pairs_parked_free", "bmh_pairs_parked_info", "bmh_pairs_parked_trim")
MEM_F_PE = 0x2

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define O(f) printf("." #f " %zu\n", offsetof(bmh_pairs_parked_info_t, f))
int main(void)
{
	printf("bmh_pairs_parked_info_t %zu\n", sizeof(bmh_pairs_parked_info_t));
	O(device); O(reads); O(regions); O(bytes);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert "typedef struct bmh_pairs_parked bmh_pairs_parked_t;" in hdr
    assert ("int bmh_pairs_sam_begin(bmh_ctx_t *ctx, const bmh_smem_opt_t *so, const bmh_chain_opt_t *co, int min_seed_len, const bmh_sam_opt_t *o, "
            "const bmh_refidx_t *bns, int n, const bmh_seq_t *seqs, uint32_t *cand /* n / 2 words, nullable */, bmh_pairs_parked_t **parked);") in hdr
    assert ("int bmh_pairs_sam_finish(bmh_ctx_t *ctx, bmh_pairs_parked_t *parked, const bmh_matesw_opt_t *mo, const bmh_sam_opt_t *o, "
            "const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t pes[4], int64_t id0, int n, const bmh_seq_t *seqs, "
            "const char *rg_id, char **text, int64_t *text_off);") in hdr
    assert "void bmh_pairs_parked_free(bmh_pairs_parked_t *parked);" in hdr
    assert "int bmh_pairs_parked_info(const bmh_pairs_parked_t *parked, bmh_pairs_parked_info_t *info);" in hdr
    assert "int bmh_pairs_parked_trim(int device);" in hdr
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    for name in ("pairs_sam_begin", "pairs_sam_finish"):
        assert callable(getattr(pkg.Context, name)), name
    nm = shutil.which("nm")
    if nm:  # exported by the library itself, and the handle's struct is no symbol of it
        syms = subprocess.run([nm, "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
        for name in SYMBOLS:
            assert name in syms, name


def test_info_layout(tmp_path):
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
    assert got == {"bmh_pairs_parked_info_t": 24, ".device": 0, ".reads": 4, ".regions": 8, ".bytes": 16}
    d = pkg.PAIRS_PARKED_INFO
    assert d.itemsize == 24 and d.names == ("device", "reads", "regions", "bytes") and [d.fields[k][1] for k in d.names] == [0, 4, 8, 16]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _begin_args(pkg, keep):
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    o["flag"] = MEM_F_PE
    so, co = np.zeros(1, dtype=pkg.SMEM_OPT), np.zeros(1, dtype=pkg.CHAIN_OPT)
    idx = pkg.make_refidx([(0, 100)], 100, [b"chr"])
    cand = np.full(4, 0xabcd, dtype=np.uint32)
    parked = C.c_void_p(0x5a5a5a5a)
    keep += [o, so, co, idx, cand, parked]
    return [None, _p(so), _p(co), 19, _p(o), C.cast(C.byref(idx), C.c_void_p), 0, None, _p(cand), C.cast(C.byref(parked), C.c_void_p)], cand, parked


def _finish_args(pkg, keep):
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    o["flag"] = MEM_F_PE
    mo = np.zeros(1, dtype=pkg.MATESW_OPT)
    idx = pkg.make_refidx([(0, 100)], 100, [b"chr"])
    pac, pes = np.zeros(25, dtype=np.uint8), np.zeros(4, dtype=pkg.PESTAT)
    text, off = C.c_void_p(0x5a5a5a5a), np.full(2, -77, dtype=np.int64)
    keep += [o, mo, idx, pac, pes, text, off]
    return [None, None, _p(mo), _p(o), C.cast(C.byref(idx), C.c_void_p), _p(pac), _p(pes), C.c_int64(0), 0, None, b"", C.cast(C.byref(text), C.c_void_p), _p(off)], text, off


def test_null_refusals():
    """a NULL context, with and without the other arguments in order: BMH_E_ARG, and *parked, the words, *text and text_off as they were"""
    pkg = load_package()
    lib = pkg.lib()
    keep = []
    args, cand, parked = _begin_args(pkg, keep)
    assert lib.bmh_pairs_sam_begin(*args) == pkg.BMH_E_ARG and parked.value == 0x5a5a5a5a and (cand == 0xabcd).all()
    for null in (1, 2, 4, 5, 8, 9):  # so, co, o, bns, cand (nullable), parked: no crash on the way to the answer
        args, cand, parked = _begin_args(pkg, keep)
        args[null] = None
        assert lib.bmh_pairs_sam_begin(*args) == pkg.BMH_E_ARG and parked.value == 0x5a5a5a5a and (cand == 0xabcd).all(), null
    args, text, off = _finish_args(pkg, keep)
    assert lib.bmh_pairs_sam_finish(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all()
    for null in (2, 3, 4, 5, 6, 11, 12):  # mo, o, bns, pac, pes, text, text_off
        args, text, off = _finish_args(pkg, keep)
        args[null] = None
        assert lib.bmh_pairs_sam_finish(*args) == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all(), null
    info = np.full(1, 7, dtype=pkg.PAIRS_PARKED_INFO)
    assert lib.bmh_pairs_parked_info(None, _p(info)) == pkg.BMH_E_ARG and (info["reads"] == 7).all()
    assert lib.bmh_pairs_finish_consumed(None) == 0


def test_free_of_null_and_trim_of_nothing():
    """bmh_pairs_parked_free(NULL) is a no-op; trimming a device that has no idle block touches no device"""
    pkg = load_package()
    lib = pkg.lib()
    assert lib.bmh_pairs_parked_free(None) is None
    assert lib.bmh_pairs_parked_free(None) is None
    assert lib.bmh_pairs_parked_trim(0) == 0 and lib.bmh_pairs_parked_trim(63) == 0
    pkg.ParkedPairs(None).free()
