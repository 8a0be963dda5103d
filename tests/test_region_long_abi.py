"""Region records of any CIGAR and MD length, their C-ABI without a GPU: the entry points are declared and exported, the record of a
long region has its 24 bytes, the version stands, bad arguments are refused before a device is needed, the Python wrappers exist,
and the preload shim refuses BMH_REGION_LONG=1 with BMH_PAC_RESIDENT=0 when it is loaded."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from __graft_entry__ import load_package

SYMBOLS = ("bmh_region_cigar_batch_long", "bmh_last_region_long_stats", "bmh_ctx_set_region_long", "bmh_last_reg2cigar_stats")


def test_region_long_symbols_sizes_version_and_null_arguments():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    for name in SYMBOLS:
        assert f"int {name}(" in hdr
        assert hasattr(lib, name)
        assert name in pkg.declared_symbols()
    for name in ("region_cigar_batch_long", "last_region_long_stats", "set_region_long", "last_reg2cigar_stats"):
        assert callable(getattr(pkg.Context, name))
    assert pkg.REGION_LONG.itemsize == 24 and pkg.REGION_LONG.names == ("region", "cigar_off", "md_off")
    assert re.search(r"typedef struct bmh_region_long \{ /\* 24 bytes \*/\s+int64_t region;[^}]*uint64_t cigar_off;[^}]*uint64_t md_off;[^}]*\} bmh_region_long_t;", hdr)
    assert "#define BMH_REGION_LONG 4u" in hdr and pkg.BMH_REGION_LONG == 4
    assert lib.bmh_version() == 310 and "#define BMH_VERSION 310" in hdr
    # refused before a device is needed: no context, and with one argument missing the outputs stay as they were
    longs, n_long, lc, lm = C.c_void_p(0x11), C.c_int64(-7), C.c_void_p(0x22), C.c_void_p(0x33)
    tail = (C.byref(longs), C.byref(n_long), C.byref(lc), C.byref(lm))
    assert lib.bmh_region_cigar_batch_long(None, None, 0, 0, None, 0, None, 0, 0, 24, 96, None, None, None, *tail) == pkg.BMH_E_ARG
    assert (longs.value, n_long.value, lc.value, lm.value) == (0x11, -7, 0x22, 0x33)
    assert lib.bmh_last_region_long_stats(None, None, None, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_region_long(None, 1) == pkg.BMH_E_ARG
    assert lib.bmh_last_reg2cigar_stats(None, None, None, None) == pkg.BMH_E_ARG


def test_shim_refuses_region_long_without_resident_reference_at_load():
    """BMH_REGION_LONG=1 with BMH_PAC_RESIDENT=0: the shim says so and leaves with status 1 when it is loaded, before any GPU work.
    Loaded into a child interpreter behind the reference library, as test_region_dedup_abi.py loads it."""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    code = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"
    env = dict(os.environ, BMH_REGION_LONG="1", BMH_PAC_RESIDENT="0")
    for k in ("BMH_REGS_DEVICE", "BMH_MATESW_DEVICE", "BMH_WANTED_DEVICE", "BMH_PHASE2_DEVICE", "BMH_PHASE2_TEXT_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert b"BMH_REGION_LONG=1" in r.stderr and b"BMH_PAC_RESIDENT must not be 0" in r.stderr and b"loaded" not in r.stdout
    env.pop("BMH_PAC_RESIDENT")
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"loaded" in r.stdout, r.stderr.decode()[-500:]
