#!/usr/bin/env python3
"""Fixture for the three paths of the exact introsort (host/sort_exact.h), produced by the COMPILED REFERENCE
(oracle/_ref/libbwa_ref.so): the region vectors and one-seed chains of tests/sortmodel.py -- McIlroy killer sequences that reach
combsort, the same with ties folded in, and structured orders -- through the reference's own mem_sort_and_dedup (bwamem.c:395) at
mask_level_redun 0.95, 0.8, 0.0 and 1.0, mem_mark_primary_se (:445) on what 0.95 leaves, and mem_chain_flt (:319) under the
default options and with mask_level / chain_drop_ratio moved.  Output: tests/golden/sort_paths_golden.npz (data only).

Every input record carries its index (regions in seedcov, chains in their position), and neither routine writes to a record it
keeps, so an output is its input thinned and permuted.  The file stores it that way -- per case the input's CRC-32 and sort keys,
per level the index list of the survivors in order -- after checking here that input[index list] IS the reference's output, byte
for byte; the tests rebuild the input from tests/sortmodel.py, check the CRC and compare bytes.  mem_mark_primary_se rewrites
fields, so its output is kept as a CRC-32 of the whole records plus the columns it decides (order, secondary, sub, sub_n).
Run in the build container:  python tools/make_sort_fixture.py"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kswlib  # noqa: E402
import reflib  # noqa: E402
import sortmodel  # noqa: E402

MARK_ID0 = 12345


def ref_dedup(L, vec, level):
    a = vec.copy()
    n = L.mem_sort_and_dedup(len(a), a.ctypes.data_as(C.c_void_p), C.c_float(level)) if len(a) else 0
    return a[:n].copy()


def ref_mark(L, opt, a, ident):
    a = a.copy()
    if len(a):
        L.mem_mark_primary_se(opt, len(a), a.ctypes.data_as(C.c_void_p), C.c_int64(ident))
    return a


def ref_chain_flt(L, opt, seeds):
    """The reference's mem_chain_flt over one-seed chains in the order given -> the seeds of the chains it keeps, in its order."""
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    n = len(seeds)
    arr = (reflib.Chain * max(n, 1))()
    for i in range(n):
        p = libc.malloc(C.sizeof(reflib.Seed) * 4)
        arr[i].n, arr[i].m, arr[i].pos = 1, 4, int(seeds[i]["rbeg"])
        arr[i].seeds = C.cast(p, C.POINTER(reflib.Seed))
        arr[i].seeds[0].rbeg, arr[i].seeds[0].qbeg, arr[i].seeds[0].len = int(seeds[i]["rbeg"]), int(seeds[i]["qbeg"]), int(seeds[i]["len"])
    m = L.mem_chain_flt(opt, n, arr)
    out = np.zeros(m, dtype=kswlib.SEED)
    for i in range(m):
        assert arr[i].n == 1
        s = arr[i].seeds[0]
        out[i] = (s.rbeg, s.qbeg, s.len)
        libc.free(C.cast(arr[i].seeds, C.c_void_p))  # (the routine freed the seeds of the chains it dropped, bwamem.c:366-371)
    return out


def main():
    L = reflib.lib()
    L.mem_sort_and_dedup.restype = C.c_int
    L.mem_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]
    L.mem_mark_primary_se.restype = None
    L.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    opt = L.mem_opt_init()
    out = {"sizes": np.array(sortmodel.SIZES, dtype=np.int32), "levels": np.array(sortmodel.LEVELS, dtype=np.float32)}
    # regions
    cases = sortmodel.region_cases()
    out["reg_names"] = np.array([name for name, _ in cases])
    out["reg_n"] = np.array([len(v) for _, v in cases], dtype=np.int32)
    out["reg_crc"] = np.array([sortmodel.crc(v) for _, v in cases], dtype=np.uint32)
    out["reg_re"] = np.concatenate([v["re"] for _, v in cases]).astype(np.int64)
    out["reg_score"] = np.concatenate([v["score"] for _, v in cases]).astype(np.int32)
    for li, level in enumerate(sortmodel.LEVELS):
        idx, cnt, marks = [], [], []
        for ci, (name, v) in enumerate(cases):
            got = ref_dedup(L, v, level)
            ix = got["seedcov"].astype(np.int64)
            assert got.tobytes() == v[ix].tobytes(), name  # the output is the input thinned and permuted
            idx.append(ix.astype(np.uint16))
            cnt.append(len(ix))
            if li == 0:
                marks.append(ref_mark(L, opt, got, MARK_ID0 + 7 * ci))
        out[f"reg_out{li}"], out[f"reg_out{li}_n"] = np.concatenate(idx), np.array(cnt, dtype=np.int32)
        if li == 0:
            out["reg_marked_crc"] = np.array([sortmodel.crc(m) for m in marks], dtype=np.uint32)
            for k in sortmodel.MARK_FIELDS:  # the order it leaves and the fields it decides, for a failure to name
                out["reg_marked_" + k] = np.concatenate([m[k] for m in marks]).astype(np.int32)
    # chains
    cases = sortmodel.chain_cases()
    out["ch_names"] = np.array([name for name, _ in cases])
    out["ch_n"] = np.array([len(s) for _, s in cases], dtype=np.int32)
    out["ch_crc"] = np.array([sortmodel.crc(s) for _, s in cases], dtype=np.uint32)
    out["ch_len"] = np.concatenate([s["len"] for _, s in cases]).astype(np.int32)
    for oi, kw in enumerate(sortmodel.CHAIN_OPTS):
        o = opt.contents
        assert (o.w, o.max_chain_gap, o.min_seed_len, o.max_occ, o.split_width) == tuple(kw[k] for k in ("w", "max_chain_gap", "min_seed_len", "max_occ", "split_width"))
        assert int(o.min_seed_len * o.split_factor + .499) == kw["split_len"]
        o.mask_level, o.chain_drop_ratio = kw["mask_level"], kw["chain_drop_ratio"]
        idx, cnt = [], []
        for name, s in cases:
            got = ref_chain_flt(L, opt, s)
            ix = got["rbeg"] // sortmodel._CH_STEP - 1
            assert got.tobytes() == s[ix].tobytes(), name
            idx.append(ix.astype(np.uint16))
            cnt.append(len(ix))
        out[f"ch_out{oi}"], out[f"ch_out{oi}_n"] = np.concatenate(idx), np.array(cnt, dtype=np.int32)
    path = os.path.join(ROOT, "tests", "golden", "sort_paths_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out["reg_names"]), "region cases,", len(out["ch_names"]), "chain cases")


if __name__ == "__main__":
    main()
