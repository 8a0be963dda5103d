"""Inputs and expectations shared by the tests of pass A of phase 2 (bmh_decide_batch on the host, bmh_decide_device on the GPU):
the committed post-processing fixture's vectors, generated pairs, the special pairs, and Python restatements of the small rules
(the selection of mem_reg2sam_se) that the composition tests hold the batch call to."""
import ctypes as C
import os

import numpy as np

import kswlib
import postgen
from __graft_entry__ import load_package
from test_postproc_cpu import sam_opt, split  # noqa: F401

L_PAC = 1_000_000  # of the fixture's pairs (tools/make_postproc_fixture.py)
SE_ID0 = 12345     # read i of the fixture was marked with id 12345 + 7 i
ID0_TRUNCATING = (2**24 - 6, 2**32 - 6, 2**33 + 2)  # pair ids (id0 >> 1) + p around 2^23, 2^31 and 2^32: mem_pair's `(int)id << 8`
PE = 0x2
NOPAIRING, ALL = 0x4, 0x8


def golden():
    return np.load(os.path.join(kswlib.GOLDEN_DIR, "postproc_golden.npz"))


def se_fixture(si):
    """(options, de-duplicated vectors, marked records flat, mapq flat) of option set si"""
    g, p = golden(), f"s{si}_"
    return sam_opt(**postgen.OPTION_SETS[si]), split(g[p + "ded"], g[p + "ded_off"]), g[p + "marked"], g[p + "mapq"]


def fixture_pes(si):
    return np.ascontiguousarray(golden()[f"s{si}_pes"], dtype=kswlib.PESTAT)


def pe_opt(si, extra_flag=0):
    o = sam_opt(**postgen.OPTION_SETS[si])
    o["flag"] = PE | extra_flag
    return o


def pe_vectors(seed, n_pairs, l_pac=L_PAC):
    return postgen.paired_vectors(np.random.default_rng(seed), n_pairs, l_pac)


def se_spread(vecs):
    """The fixture's reads were marked with ids 12345 + 7 i and a batch numbers its reads consecutively: read i goes to place 7 i of
    a batch that starts at 12345, with empty vectors between."""
    out = [np.zeros(0, dtype=kswlib.ALNREG) for _ in range(7 * len(vecs))]
    for i, v in enumerate(vecs):
        out[7 * i] = v
    return out


def want_se_py(o, a):
    """bwamem.c:1057-1062 with the library's rb < 0 || re < 0 rule, over a marked vector"""
    out = []
    for k in range(len(a)):
        p = a[k]
        if int(p["score"]) < int(o["T"]):
            continue
        sec = int(p["secondary"])
        if sec >= 0 and not (int(o["flag"]) & ALL):
            continue
        if sec >= 0 and float(int(p["score"])) < float(int(a[sec]["score"])) * .5:
            continue
        if int(p["rb"]) < 0 or int(p["re"]) < 0:
            continue
        out.append(k)
    return out


def lib_pair(L, o, l_pac, pes, a0, a1, ident):
    """bmh_pair over two marked vectors -> (score, sub, n_sub, z0, z1); z stays (-1, -1) where it finds nothing"""
    L.bmh_pair.restype = C.c_int
    c_regs = kswlib.regs_to_c([a0, a1])
    sub, nsub = C.c_int(0), C.c_int(0)
    z = (C.c_int * 2)(-1, -1)
    oo = L.bmh_pair(o.ctypes.data_as(C.c_void_p), C.c_int64(l_pac), pes.ctypes.data_as(C.c_void_p), c_regs, C.c_uint64(ident), C.byref(sub), C.byref(nsub), z)
    kswlib.regs_from_c(c_regs)
    return oo, sub.value, nsub.value, z[0], z[1]


def lib_mark(L, o, a, ident):
    a = np.array(a, dtype=kswlib.ALNREG, copy=True)
    L.bmh_mark_primary_se.restype = None
    L.bmh_mark_primary_se(o.ctypes.data_as(C.c_void_p), C.c_int(len(a)), a.ctypes.data_as(C.c_void_p), C.c_int64(ident))
    return a


def check_pe_composition(L, o, l_pac, pes, id0, vecs, out):
    """A PE result against the single routines: mem_pair's figures, and the want lists against want_se_py.  Returns how many pairs
    were decided as pairs and how many of those the pair itself won."""
    n_paired = n_won = 0
    for p in range(len(vecs) // 2):
        pid = (id0 >> 1) + p
        m = [lib_mark(L, o, vecs[2 * p + r], pid << 1 | r) for r in range(2)]
        d = out["pd"][p]
        asked = not (int(o["flag"]) & NOPAIRING) and len(m[0]) and len(m[1])
        oo, sub, nsub, z0, z1 = lib_pair(L, o, l_pac, pes, m[0], m[1], pid) if asked else (0, 0, 0, -1, -1)
        assert (int(d["score"]), int(d["sub"]), int(d["n_sub"])) == (oo, sub, nsub), (p, d, (oo, sub, nsub))
        # z is mem_pair's unless the two best single-end hits won (then it is 0, 0 by mem_sam_pe's rule) or nothing was found
        singles_won = int(d["paired"]) and not (int(d["extra_flag"]) & 2)
        if oo > 0 and not singles_won:
            assert tuple(d["z"]) == (z0, z1), (p, d, z0, z1)
        if singles_won or oo == 0:
            assert tuple(d["z"]) == (0, 0), (p, d)
        n_paired += int(d["paired"])
        n_won += int(d["paired"]) and bool(int(d["extra_flag"]) & 2)
        for r in range(2):
            a = out["regs"][2 * p + r]
            if int(d["paired"]):
                k = int(d["z"][r])
                want = [k] if int(a[k]["rb"]) >= 0 and int(a[k]["re"]) >= 0 else []
            else:
                want = want_se_py(o, a)
                # nothing but a winning pair touches the marked vectors
                assert a.tobytes() == m[r].tobytes(), (p, r)
            assert list(out["want"][2 * p + r]) == want, (p, r, list(out["want"][2 * p + r]), want)
    return n_paired, n_won


def assert_same(dev, host, what=""):
    """device result against host result: regions byte for byte, pd, reg_mapq, n_want, want_k"""
    assert len(dev["regs"]) == len(host["regs"])
    for i, (a, b) in enumerate(zip(dev["regs"], host["regs"])):
        assert a.tobytes() == b.tobytes(), f"{what}: regions of read {i} differ\ndevice={a}\nhost={b}"
    for k in ("pd", "reg_mapq", "n_want", "want_k"):
        assert dev[k].tobytes() == host[k].tobytes(), f"{what}: {k} differs at {np.nonzero(np.atleast_1d(dev[k] != host[k]))[0][:8]}"


def special_pes(kind):
    """all four orientations failed / one open orientation with std = 0 / the fixture's"""
    pes = fixture_pes(0).copy()
    if kind == "none":
        pes["failed"] = 1
    elif kind == "std0":
        pes["failed"] = 1
        pes[1]["failed"], pes[1]["std"] = 0, 0.0
    elif kind == "wide":  # a window of 2^21 distances: the pair table would pass 2^20 entries
        pes[1]["low"], pes[1]["high"] = 1, 1 + (1 << 21)
    return pes


def vectors_of_sizes(rng, sizes, l_pac=3_000_000):
    """one region vector of each size, drawn like postgen.region_vectors' (ties in score, overlaps)"""
    out = []
    while len(out) < len(sizes):
        n = sizes[len(out)]
        pool = [r for v in postgen.region_vectors(rng, 40, l_pac) for r in v]
        a = np.array(pool[:n], dtype=kswlib.ALNREG) if n else np.zeros(0, dtype=kswlib.ALNREG)
        assert len(a) == n
        out.append(a)
    return out
