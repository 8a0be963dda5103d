"""The device chainer's C-ABI without a GPU: the entry points are declared and exported, reject bad arguments before they touch a
device, and the header's chaining comments name them."""
import ctypes as C

import numpy as np

from __graft_entry__ import load_package
from test_chain_cpu import CHAIN_OPT


def test_device_chainer_symbols_and_argument_checks():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    for name in ("bmh_chain_batch", "bmh_seed_chain_batch", "bmh_chain_stats"):
        assert f"int {name}(" in hdr
        assert hasattr(lib, name)
    assert "stays host code" not in hdr
    o = np.zeros((), dtype=CHAIN_OPT)
    # no context: BMH_E_ARG, nothing else happens
    assert lib.bmh_chain_batch(None, o.ctypes.data_as(C.c_void_p), C.c_int64(0), 0, None, None, None, None, None, None, None,
                               C.c_uint64(0), None) == pkg.BMH_E_ARG
    assert lib.bmh_seed_chain_batch(None, None, o.ctypes.data_as(C.c_void_p), C.c_int64(0), 0, None, None) == pkg.BMH_E_ARG
    assert lib.bmh_chain_stats(None, None) == pkg.BMH_E_ARG
