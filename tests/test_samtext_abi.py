"""The C-ABI of pass C of phase 2 without a GPU: bmh_sam_text_batch, bmh_sam_text_device, the resident names, the context switch and
its statistics are declared and exported, bmh_samtext_stats_t keeps its 56-byte layout, and bad arguments are refused before a device
is touched.  With a device: the statistics before the first call, and the refusals without the resident tables."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
import samtextgen as sg
from __graft_entry__ import load_package

FIELDS = ("reads", "lines", "text_bytes", "h2d_bytes", "d2h_bytes", "waits", "size_ms", "emit_ms")
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
	S(bmh_samtext_stats_t); O(bmh_samtext_stats_t, reads); O(bmh_samtext_stats_t, lines); O(bmh_samtext_stats_t, text_bytes);
	O(bmh_samtext_stats_t, h2d_bytes); O(bmh_samtext_stats_t, d2h_bytes); O(bmh_samtext_stats_t, waits); O(bmh_samtext_stats_t, size_ms);
	O(bmh_samtext_stats_t, emit_ms); S(bmh_seq_t); S(bmh_refann_t);
	printf("BMH_VERSION %d\n", BMH_VERSION);
	return 0;
}
"""
ARGS = ("const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const bmh_pestat_t *pes, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs, "
        "const int64_t *roff, const bmh_pairdec_t *pd, const int32_t *reg_mapq, const int32_t *n_want, const int32_t *want_k, "
        "const bmh_wanted_res_t *results, const uint32_t *cigar_pool, const char *md_pool, const char *rg_id, char **text, int64_t *text_off);")


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert "int bmh_sam_text_batch(" + ARGS in hdr
    assert "int bmh_sam_text_device(bmh_ctx_t *ctx, " + ARGS in hdr
    assert "int bmh_ctx_set_refnames(bmh_ctx_t *ctx, const bmh_refidx_t *bns);" in hdr
    assert "int bmh_ctx_set_samtext_device(bmh_ctx_t *ctx, int on);" in hdr
    assert "int bmh_last_samtext_stats(const bmh_ctx_t *ctx, bmh_samtext_stats_t *st);" in hdr
    for name in ("bmh_sam_text_batch", "bmh_sam_text_device", "bmh_ctx_set_refnames", "bmh_ctx_set_samtext_device", "bmh_last_samtext_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    for name in ("bmh_samtext_check_", "bmh_samtext_routed_"):  # between the library's own files
        assert not hasattr(lib, name), name
    for name in ("sam_text_batch", "set_refnames", "set_samtext_device", "last_samtext_stats"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.sam_text_batch)
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
    want = {"bmh_samtext_stats_t": 56, "bmh_seq_t": C.sizeof(pkg._Seq), "bmh_refann_t": C.sizeof(pkg._RefAnn), "BMH_VERSION": 310}
    for name in FIELDS:
        want["bmh_samtext_stats_t." + name] = pkg.SAMTEXT_STATS.fields[name][1]
    assert got == want
    assert pkg.SAMTEXT_STATS.itemsize == 56
    assert [pkg.SAMTEXT_STATS.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_refusals_without_a_context():
    pkg = load_package()
    lib = pkg.lib()
    idx = sg.refidx()
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    t, off = C.c_void_p(0x5a5a5a5a), np.full(1, -77, dtype=np.int64)
    st = np.full(1, 7, dtype=pkg.SAMTEXT_STATS)
    rc = lib.bmh_sam_text_device(None, o.ctypes.data, C.byref(idx), None, 0, *([None] * 10), b"", C.byref(t), off.ctypes.data)
    assert rc == pkg.BMH_E_ARG and t.value == 0x5a5a5a5a and off[0] == -77
    assert lib.bmh_ctx_set_refnames(None, C.byref(idx)) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_refnames(None, None) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_samtext_device(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_samtext_stats(None, st.ctypes.data) == pkg.BMH_E_ARG
    assert (st["reads"] == 7).all()
    # the host form needs no context: no read gives an empty pool
    assert lib.bmh_sam_text_batch(o.ctypes.data, C.byref(idx), None, 0, *([None] * 10), b"", C.byref(t), off.ctypes.data) == 0
    assert off[0] == 0 and t.value not in (None, 0x5a5a5a5a)
    pkg._libc.free(t)


def test_with_a_context_before_the_first_call_and_without_the_tables():
    """every field -1 on a fresh context, and the device call refused while a table is missing; without a device the context is refused
    loudly, which is all there is to see"""
    pkg = load_package()
    try:
        c = pkg.Context(0, kswlib.make_params())
    except pkg.BmhError as e:
        assert e.code == pkg.BMH_E_NODEVICE
        return
    try:
        st = c.last_samtext_stats()
        assert tuple(st) == FIELDS and all(v == -1 for v in st.values()), st
        c.set_samtext_device(True), c.set_samtext_device(False)
        assert all(v == -1 for v in c.last_samtext_stats().values())
        sl = sg.make("se", 5, seed=1)
        idx = sg.refidx()
        args = (sl["opt"], idx, sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"], sl["cig"], sl["md"], sl["rg_id"])
        for setup in ((), ("set_refidx",), ("set_refnames",)):
            c.set_refidx(None), c.set_refnames(None)
            for f in setup:
                getattr(c, f)(idx)
            out = sg.sentinels(5)
            with pytest.raises(pkg.BmhError) as e:
                c.sam_text_batch(*args, out=out)
            assert e.value.code == pkg.BMH_E_ARG and out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all(), setup
        c.set_refidx(idx), c.set_refnames(idx)
        other = pkg.make_refidx([(o, n) for o, n in sg.CONTIGS], sg.L_PAC, [b"x" + nm for nm in sg.NAMES])
        with pytest.raises(pkg.BmhError) as e:  # the names of another reference
            c.sam_text_batch(sl["opt"], other, *args[2:])
        assert e.value.code == pkg.BMH_E_ARG
        text, off = c.sam_text_batch(*args)
        assert (text, off.tolist()) == tuple((lambda t, o: (t, o.tolist()))(*pkg.sam_text_batch(*args)))
    finally:
        c.close()
