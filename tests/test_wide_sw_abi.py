"""The wide Smith-Waterman's C-ABI without a GPU: both entry points are exported and declared, reject a missing context, the
binding's methods exist, and the library version is unchanged."""
import ctypes as C

from __graft_entry__ import load_package


def test_wide_sw_symbols_and_version():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    assert "int bmh_ctx_set_wide_sw(bmh_ctx_t *ctx, int enable);" in hdr
    assert "int bmh_sw_wide_stats(const bmh_ctx_t *ctx, int64_t *tasks, float *ms);" in hdr
    for name in ("bmh_ctx_set_wide_sw", "bmh_sw_wide_stats"):
        assert hasattr(lib, name) and name in pkg.declared_symbols()
    assert lib.bmh_version() == 310 and "#define BMH_VERSION 310 " in hdr
    n, ms = C.c_int64(7), C.c_float(0)
    assert lib.bmh_ctx_set_wide_sw(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_wide_sw(None, 0) == pkg.BMH_E_ARG
    assert lib.bmh_sw_wide_stats(None, C.byref(n), C.byref(ms)) == pkg.BMH_E_ARG
    ctx = pkg.Context.__new__(pkg.Context)
    assert callable(ctx.set_wide_sw) and callable(ctx.sw_wide_stats)
