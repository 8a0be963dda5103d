"""Region de-duplication on the device, its C-ABI without a GPU: the three entry points are declared and exported, reject a NULL
context before they touch a device, the Python wrappers exist, and the preload shim refuses BMH_DEDUP_DEVICE=1 without
BMH_REGS_DEVICE=1 when it is loaded."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from __graft_entry__ import load_package

SYMBOLS = ("bmh_sort_dedup_batch", "bmh_ctx_set_regs_dedup", "bmh_last_dedup_stats")


def test_dedup_symbols_wrappers_and_null_context():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    for name in SYMBOLS:
        assert f"int {name}(" in hdr
        assert hasattr(lib, name)
        assert name in pkg.declared_symbols()
    for name in ("sort_dedup_batch", "set_regs_dedup", "last_dedup_stats"):
        assert callable(getattr(pkg.Context, name))
    assert lib.bmh_sort_dedup_batch(None, 0, None, C.c_float(0.95)) == pkg.BMH_E_ARG
    assert lib.bmh_ctx_set_regs_dedup(None, 1, C.c_float(0.95)) == pkg.BMH_E_ARG
    assert lib.bmh_last_dedup_stats(None, None, None, None) == pkg.BMH_E_ARG


def test_shim_refuses_dedup_device_without_regs_device_at_load():
    """BMH_DEDUP_DEVICE=1 alone: the shim says so and leaves with status 1 when it is loaded, before any GPU work.  Loaded into a
    child interpreter behind the reference library, as test_chain2reg_abi.py loads it."""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    code = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"
    env = dict(os.environ, BMH_DEDUP_DEVICE="1")
    env.pop("BMH_REGS_DEVICE", None)
    env.pop("BMH_PAC_RESIDENT", None)
    for regs in (None, "0"):
        if regs is not None:
            env["BMH_REGS_DEVICE"] = regs
        r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
        assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
        assert b"BMH_DEDUP_DEVICE=1" in r.stderr and b"needs BMH_REGS_DEVICE=1" in r.stderr and b"loaded" not in r.stdout
    env["BMH_REGS_DEVICE"] = "1"
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"loaded" in r.stdout, r.stderr.decode()[-500:]
    # the check beside it still answers first for its own contradiction
    env["BMH_PAC_RESIDENT"] = "0"
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"BMH_PAC_RESIDENT must not be 0" in r.stderr
