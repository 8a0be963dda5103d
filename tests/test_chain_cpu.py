"""Seeds to chains (bmh_chain_reads) is host code: compared here, on the CPU, with the chains the
COMPILED REFERENCE's mem_chain + mem_chain_flt produced for the same reads (tests/golden/chain_golden.npz,
tools/make_chain_fixture.py): same chains, same seeds, same ORDER -- on a repeat-rich genome where a read has up to
dozens of chains, so that the B-tree of chains splits and equal keys / equal weights occur."""
import ctypes as C
import os

import numpy as np
import pytest

import kswlib
from __graft_entry__ import load_package

BMH_E_ARG = -3
CHAIN_OPT = np.dtype([("w", "<i4"), ("max_chain_gap", "<i4"), ("min_seed_len", "<i4"), ("max_occ", "<i4"), ("split_len", "<i4"),
                      ("split_width", "<i4"), ("mask_level", "<f4"), ("chain_drop_ratio", "<f4")])


class _Read(C.Structure):
    _fields_ = [("l_seq", C.c_int32), ("seq", C.c_void_p)]


class _Chain(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("pos", C.c_int64), ("seeds", C.c_void_p)]


class _ChainV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(_Chain))]


def chain_tables(lib, o, reads, calls, intvs, sa_k, sa_pos):
    """The flat tables bmh_chain_reads takes; the suffix-array positions in interval order, as the library's own key list asks
    for them (one bmh_sa_batch on the GPU in production; here they come out of the fixture's sorted table)."""
    n = len(reads)
    t = {"reads": reads}
    t["call_off"] = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint32)
    t["intv_off"] = np.concatenate([[0], np.cumsum([len(v) for v in intvs])]).astype(np.uint64)
    t["calls"] = np.ascontiguousarray(np.concatenate(calls)) if n else np.zeros(0, kswlib.SMEM_CALL)
    fi = t["intv"] = np.ascontiguousarray(np.concatenate(intvs)) if n else np.zeros(0, kswlib.SMEM_INTV)
    lib.bmh_chain_sa_keys.restype = C.c_uint64
    sa_off = t["sa_off"] = np.zeros(len(fi) + 1, dtype=np.uint64)
    nk = lib.bmh_chain_sa_keys(o.ctypes.data_as(C.c_void_p), C.c_uint64(len(fi)), fi.ctypes.data_as(C.c_void_p), sa_off.ctypes.data_as(C.c_void_p), None)
    keys = np.zeros(nk + 1, dtype=np.uint64)
    assert lib.bmh_chain_sa_keys(o.ctypes.data_as(C.c_void_p), C.c_uint64(len(fi)), fi.ctypes.data_as(C.c_void_p), sa_off.ctypes.data_as(C.c_void_p),
                                 keys.ctypes.data_as(C.c_void_p)) == nk
    at = np.searchsorted(sa_k, keys[:nk])
    assert (sa_k[at] == keys[:nk]).all()
    t["sa_pos"] = np.ascontiguousarray(np.concatenate([sa_pos[at], np.zeros(1, np.uint64)]))
    return t


def call_chain_reads(lib, o, l_pac, t):
    """bmh_chain_reads over chain_tables' output: (return code, the bmh_chain_v array)."""
    reads = t["reads"]
    n = len(reads)
    c_reads = (_Read * n)()
    for k, r in enumerate(reads):
        c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
    out = (_ChainV * n)()
    rc = lib.bmh_chain_reads(o.ctypes.data_as(C.c_void_p), C.c_int64(l_pac), C.c_int(n), C.cast(c_reads, C.c_void_p),
                             *[t[k].ctypes.data_as(C.c_void_p) for k in ("call_off", "calls", "intv_off", "intv", "sa_off", "sa_pos")],
                             C.cast(out, C.c_void_p))
    return rc, out


def run_chain_reads(lib, o, l_pac, reads, calls, intvs, sa_k, sa_pos):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    rc, out = call_chain_reads(lib, o, l_pac, chain_tables(lib, o, reads, calls, intvs, sa_k, sa_pos))
    assert rc == 0, rc
    res = []
    for k in range(len(reads)):
        chains = []
        assert out[k].n <= out[k].m and (out[k].m == 0) == (not out[k].a)
        for ci in range(out[k].n):
            c = out[k].a[ci]
            assert c.m == max(4, 1 << (c.n - 1).bit_length())  # capacities as mem_insert_seed grows them: 4, 8, 16, ...
            sd = np.zeros(c.n, dtype=kswlib.SEED)
            C.memmove(sd.ctypes.data, c.seeds, c.n * kswlib.SEED.itemsize)
            assert c.pos == sd["rbeg"][0]
            chains.append(sd)
            libc.free(c.seeds)
        if out[k].a:
            libc.free(C.cast(out[k].a, C.c_void_p))
        res.append(chains)
    return res


def fixture_groups():
    """(name, options, l_pac, reads, calls, intervals, sa_k, sa_pos, n_chains per read, flat chain seed lists) per group."""
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "chain_golden.npz"))
    l_pac = int(g["l_pac"])
    cut = lambda flat, cnt: np.split(flat, np.cumsum(cnt)[:-1])
    for p in [str(x) for x in g["groups"]]:
        o = np.zeros((), dtype=CHAIN_OPT)
        for f, v in zip(CHAIN_OPT.names[:6], g[p + "opt"]):
            o[f] = v
        o["mask_level"], o["chain_drop_ratio"] = g[p + "optf"]
        reads = [np.ascontiguousarray(r) for r in cut(g[p + "reads"], g[p + "read_len"])]
        calls, intvs = cut(g[p + "calls"], g[p + "n_calls"]), cut(g[p + "intv"], g[p + "n_intv"])
        nseeds = cut(g[p + "seeds"], g[p + "n_seeds"]) if len(g[p + "n_seeds"]) else []
        yield (p, o, l_pac, reads, calls, intvs, np.ascontiguousarray(g[p + "sa_k"]), np.ascontiguousarray(g[p + "sa_pos"]),
               g[p + "n_chains"], nseeds)


def test_chains_match_reference_fixture():
    lib = load_package().lib()
    lib.bmh_chain_reads.restype = C.c_int
    total, deep = 0, 0
    for p, o, l_pac, reads, calls, intvs, sa_k, sa_pos, n_chains, nseeds in fixture_groups():
        got = run_chain_reads(lib, o, l_pac, reads, calls, intvs, sa_k, sa_pos)
        it = iter(nseeds)
        for r, nch in enumerate(n_chains):
            want = [next(it) for _ in range(int(nch))]
            assert len(got[r]) == len(want), f"{p} read {r}: {len(got[r])} chains, reference {len(want)}"
            for ci, (a, b) in enumerate(zip(got[r], want)):
                assert len(a) == len(b) and (a == b).all(), f"{p} read {r} chain {ci}: ours={a} ref={b}"
            total += len(want)
            deep += len(want) > 15
    assert total == 4289 and deep > 30  # reads whose chains split the B-tree's root (more than 2t-1 = 15 keys)


def test_inconsistent_tables_leave_no_chains():
    """Three corruptions of the fixture's tables, each in a read after others that chain: BMH_E_ARG, and no read keeps chains."""
    lib = load_package().lib()
    lib.bmh_chain_reads.restype = C.c_int
    p, o, l_pac, reads, calls, intvs, sa_k, sa_pos, n_chains, _ = next(fixture_groups())
    rc, out = call_chain_reads(lib, o, l_pac, chain_tables(lib, o, reads, calls, intvs, sa_k, sa_pos))
    assert rc == 0 and all(out[r].n for r in range(10))
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for r in range(len(reads)):
        for ci in range(out[r].n):
            libc.free(out[r].a[ci].seeds)
        libc.free(C.cast(out[r].a, C.c_void_p))
    ilen = lambda v: int((v["info"] & 0xFFFFFFFF) - (v["info"] >> 32))
    long_rare = lambda v: ilen(v) >= int(o["min_seed_len"]) and int(v["x2"]) <= int(o["max_occ"])

    def reseed_call():  # a call that re-seeds its predecessor (smem_next2's order), in a read past the tenth
        for r in range(10, len(reads)):
            split_len = min(int(o["split_len"]), len(reads[r]))
            c = 0
            while c < len(calls[r]):
                mc = calls[r][c]
                m = intvs[r][int(mc["first"]): int(mc["first"]) + int(mc["n"])]
                lens = [ilen(v) for v in m]
                c += 1
                if len(m) and split_len > 0 and max(lens) >= split_len and int(m[int(np.argmax(lens))]["x2"]) <= int(o["split_width"]):
                    return r, c
        raise AssertionError("no re-seeding call in the fixture")

    def corrupt(kind):
        t = chain_tables(lib, o, reads, calls, intvs, sa_k, sa_pos)
        if kind == "reseed_x":
            r, c = reseed_call()
            t["calls"]["x"][int(t["call_off"][r]) + c] += 1
        elif kind == "sa_off":
            r, k = next((r, int(c0["first"]) + i) for r in range(10, len(reads)) if len(reads[r]) >= int(o["min_seed_len"]) and len(calls[r])
                        for c0 in calls[r][:1] for i in range(int(c0["n"])) if long_rare(intvs[r][int(c0["first"]) + i]))  # a main call's
            t["sa_off"][int(t["intv_off"][r]) + k] = np.iinfo(np.uint64).max
        else:  # a call whose intervals run past the read's own
            r = next(r for r in range(10, len(reads)) if len(reads[r]) >= int(o["min_seed_len"]) and len(calls[r]))
            t["calls"]["n"][int(t["call_off"][r])] = len(intvs[r]) - int(calls[r][0]["first"]) + 1
        return t

    for kind in ("reseed_x", "sa_off", "call_range"):
        rc, out = call_chain_reads(lib, o, l_pac, corrupt(kind))
        assert rc == BMH_E_ARG, (kind, rc)
        assert all(out[r].n == 0 and out[r].m == 0 and not out[r].a for r in range(len(reads))), kind
