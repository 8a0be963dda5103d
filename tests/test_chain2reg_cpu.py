"""host/chain2aln_core.h, the arithmetic the host and device chains-to-regions drivers share, as the library compiled it:
cal_max_gap (two double divisions, bwamem.c:544-551) against the oracle's restatement under every parameter set of the
mem_chain2aln fixture."""
import ctypes as C

import numpy as np

import kswlib
from __graft_entry__ import load_package


def test_shared_cal_max_gap_equals_the_oracle():
    lib, orc = load_package().lib(), kswlib.load_oracle()
    lib.bmh_cal_max_gap_.restype = C.c_int
    lib.bmh_cal_max_gap_.argtypes = [C.c_void_p, C.c_int]
    orc.orc_cal_max_gap.restype = C.c_int
    orc.orc_cal_max_gap.argtypes = [C.c_void_p, C.c_int]
    params = kswlib.load_golden("chain2aln_golden.npz")["params"]
    assert len(params) >= 2
    seen = set()
    for p in params:
        p = np.ascontiguousarray(np.asarray(p, dtype=kswlib.PARAMS).reshape(()))
        ptr = p.ctypes.data_as(C.c_void_p)
        for q in range(0, 70001):
            a, b = lib.bmh_cal_max_gap_(ptr, q), orc.orc_cal_max_gap(ptr, q)
            assert a == b, (p, q, a, b)
            seen.add(a)
    assert len(seen) > 50  # below the 2*w cap the value moves with qlen
