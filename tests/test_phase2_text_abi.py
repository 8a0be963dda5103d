"""The C-ABI of the session that runs passes A, B and C of phase 2 without a GPU: bmh_phase2_text_device, its switch and
bmh_last_phase2_text_stats are declared and exported, bmh_phase2_text_stats_t keeps its 112-byte layout, and a NULL context is refused
before a device is touched.  (With a context the same refusals are tests/test_phase2_text_device_gpu.py's.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

FIELDS = ("units", "wanted", "fixed", "redone", "reads", "lines", "text_bytes", "h2d_bytes", "d2h_bytes", "fallbacks", "waits", "sessions",
          "decide_ms", "wanted_ms", "gather_ms", "size_ms", "emit_ms")
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 92, 96, 100, 104]

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwamem_hip.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(f) printf("." #f " %zu\n", offsetof(bmh_phase2_text_stats_t, f))
int main(void)
{
	S(bmh_phase2_text_stats_t); O(units); O(wanted); O(fixed); O(redone); O(reads); O(lines); O(text_bytes); O(h2d_bytes); O(d2h_bytes);
	O(fallbacks); O(waits); O(sessions); O(decide_ms); O(wanted_ms); O(gather_ms); O(size_ms); O(emit_ms); O(rsv_);
	S(bmh_phase2_stats_t); S(bmh_samtext_stats_t);
	return 0;
}
"""


def test_header_text_and_exported_symbols():
    pkg = load_package()
    lib = pkg.lib()
    hdr = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("int bmh_phase2_text_device(bmh_ctx_t *ctx, const bmh_sam_opt_t *o, const bmh_refidx_t *bns, const uint8_t *pac, const bmh_pestat_t *pes, "
            "int64_t id0, int n, const bmh_seq_t *seqs, const bmh_alnreg_v *regs, const char *rg_id, char **text, int64_t *text_off);") in hdr
    assert "int bmh_ctx_set_phase2_text_device(bmh_ctx_t *ctx, int on);" in hdr
    assert "int bmh_last_phase2_text_stats(const bmh_ctx_t *ctx, bmh_phase2_text_stats_t *st);" in hdr
    for name in ("bmh_phase2_text_device", "bmh_ctx_set_phase2_text_device", "bmh_last_phase2_text_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols(), name
    # the hooks between the library's own translation units are not part of the interface
    assert not hasattr(lib, "bmh_phase2_text_routed_") and not hasattr(lib, "bmh_samtext_check_seqs_")
    for name in ("phase2_text_device", "set_phase2_text_device", "last_phase2_text_stats"):
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
    want = {"bmh_phase2_text_stats_t": 112, "bmh_phase2_stats_t": 72, "bmh_samtext_stats_t": 56, ".rsv_": 108}
    for name in FIELDS:
        want["." + name] = pkg.PHASE2_TEXT_STATS.fields[name][1]
    assert got == want
    assert pkg.PHASE2_TEXT_STATS.itemsize == 112 and pkg.PHASE2_TEXT_STATS.names == FIELDS + ("rsv",)
    assert [pkg.PHASE2_TEXT_STATS.fields[k][1] for k in FIELDS] == OFFSETS


def test_refusals_without_a_context():
    """a NULL context, with everything else in order and with what the call refuses besides: a NULL text or text_off, odd n with PE"""
    pkg = load_package()
    lib = pkg.lib()
    o = np.zeros(1, dtype=pkg.SAM_OPT)
    pe = o.copy()
    pe["flag"] = pkg.MEM_F_PE
    text = C.c_void_p(0x5a5a5a5a)
    off = np.full(2, -77, dtype=np.int64)
    tp, op = C.cast(C.byref(text), C.c_void_p), off.ctypes.data_as(C.c_void_p)
    for opt, n, t, f in ((o, 0, tp, op), (o, 0, None, op), (o, 0, tp, None), (pe, 1, tp, op)):
        rc = lib.bmh_phase2_text_device(None, opt.ctypes.data_as(C.c_void_p), None, None, None, C.c_int64(0), n, None, None, b"", t, f)
        assert rc == pkg.BMH_E_ARG and text.value == 0x5a5a5a5a and (off == -77).all()
    st = np.full(1, 7, dtype=pkg.PHASE2_TEXT_STATS)
    assert lib.bmh_ctx_set_phase2_text_device(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_phase2_text_stats(None, st.ctypes.data_as(C.c_void_p)) == pkg.BMH_E_ARG
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
        st = c.last_phase2_text_stats()
        assert tuple(st) == FIELDS and all(v == -1 for v in st.values()), st
        c.set_phase2_text_device(True), c.set_phase2_text_device(False)
        assert all(v == -1 for v in c.last_phase2_text_stats().values())
    finally:
        c.close()
