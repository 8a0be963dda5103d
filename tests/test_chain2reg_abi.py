"""The chains-to-regions device driver's C-ABI without a GPU: both entry points are declared and exported, reject bad arguments
before they touch a device, the Python wrappers exist, and a context still cannot be made without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package
from test_chain_cpu import CHAIN_OPT


def test_chain2reg_symbols_and_argument_checks():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    for name in ("bmh_chains2regs_device", "bmh_seed_chain_regs_batch"):
        assert f"int {name}(" in hdr
        assert hasattr(lib, name)
    for name in ("chains2regs_device", "seed_chain_regs_batch", "chains2regs_batch"):
        assert callable(getattr(pkg.Context, name))
    o = np.zeros((), dtype=CHAIN_OPT)
    so = np.zeros((), dtype=kswlib.SMEM_OPT)
    # no context: BMH_E_ARG, nothing else happens
    assert lib.bmh_chains2regs_device(None, C.c_int64(0), 0, None, None, 0, None) == pkg.BMH_E_ARG
    assert lib.bmh_seed_chain_regs_batch(None, so.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), C.c_int64(0), 0, None, 0,
                                         None) == pkg.BMH_E_ARG
    assert lib.bmh_seed_chain_regs_batch(None, None, None, C.c_int64(0), 0, None, 0, None) == pkg.BMH_E_ARG


def test_no_gpu_still_means_no_context():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    pkg = load_package()
    with pytest.raises(pkg.BmhError) as e:
        pkg.Context(0, kswlib.make_params())
    assert e.value.code == pkg.BMH_E_NODEVICE


def test_shim_refuses_regs_device_without_resident_reference_at_load():
    """BMH_REGS_DEVICE=1 with BMH_PAC_RESIDENT=0: the shim says so and leaves with status 1 when it is loaded, before any GPU work.
    Loaded into a child interpreter behind the reference library, as test_align1_core_gpu.py loads it."""
    import reflib
    pkg = load_package()
    if not reflib.have_ref_bwa() or not os.path.exists(pkg.DROPIN_PATH):
        pytest.skip("oracle/_ref not built")
    code = "import ctypes as C, sys; C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL); C.CDLL(sys.argv[2]); print('loaded')"
    env = dict(os.environ, BMH_REGS_DEVICE="1", BMH_PAC_RESIDENT="0")
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert b"BMH_PAC_RESIDENT must not be 0" in r.stderr and b"loaded" not in r.stdout
    env["BMH_PAC_RESIDENT"] = "1"
    r = subprocess.run([sys.executable, "-c", code, reflib.REF_LIB, pkg.DROPIN_PATH], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"loaded" in r.stdout, r.stderr.decode()[-500:]
