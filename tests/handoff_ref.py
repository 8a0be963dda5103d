"""What phase 2 must know of a batch's regions before its first launch, restated plainly from csrc/api.hip's decide_table_sizes
(the single-end part) and oriented_cap as they stood before host/handoff_core.h: for tests/test_handoff_core_cpu.py and
tests/test_reads_sam_device_gpu.py.  Nothing here reads the header."""
import numpy as np

import kswlib

ALNREG = kswlib.ALNREG


def _i32(x):
    return int(np.int64(x).astype(np.int32))


def pp_len(a):
    """bmh_pp_len: the longer of the two spans, in int arithmetic (the reference span converted to int)"""
    q = _i32(int(a["qe"]) - int(a["qb"]))
    r = int(a["re"]) - int(a["rb"])
    return q if q > r else _i32(r)


def plan(o, vecs):
    """(kmax or None where decide_table_sizes refuses a negative index, opool_cap, total, refused) over per-read ALNREG arrays"""
    mcl = np.float32(o["mapQ_coef_len"])
    kmax, cap, total, refused = 1, 0, 0, False
    for v in vecs:
        nv = len(v)
        total += nv
        for a in v:
            idx = 0
            if mcl > 0:
                ln = pp_len(a)
                if not np.float32(ln) < mcl:
                    idx = ln
            else:
                idx = int(a["seedcov"])
            if idx < 0:
                refused = True
            else:
                kmax = max(kmax, idx, max(int(a["sub_n"]), 0) + nv + 1)
            cap += min(max(int(a["qe"]) - int(a["qb"]), 0), 65535) + min(max(int(a["re"]) - int(a["rb"]), 0), 65535)
    return (None if refused else kmax), cap, total, refused


def random_vectors(rng, n_reads, l_pac=3_000_000, neg_seedcov=False):
    """Seeded vectors for every clause of the rule: empty vectors, vectors of 1 to 40, sub_n negative and large, lengths on both sides
    of mapQ_coef_len = 50, spans that are negative and past 65535 on either side; neg_seedcov: a few regions with seedcov < 0"""
    vecs = []
    for r in range(n_reads):
        k = int(rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 40]))
        v = np.zeros(k, dtype=ALNREG)
        for a in v:
            kind = int(rng.integers(0, 10))
            rb = int(rng.integers(0, 2 * l_pac - 200_000))
            qb = int(rng.integers(0, 200))
            ql = int(rng.integers(1, 49)) if kind == 0 else int(rng.integers(50, 400))  # (below mapQ_coef_len: neither span reaches it)
            rl = ql + int(rng.integers(-5, 6)) if kind else int(rng.integers(1, 49))
            if kind == 1:
                ql = -int(rng.integers(1, 300))  # qe < qb
            elif kind == 2:
                rl = -int(rng.integers(1, 300))  # re < rb
            elif kind == 3:
                ql = 65_535 + int(rng.integers(-1, 500))  # at and past the cap
            elif kind == 4:
                rl = 65_535 + int(rng.integers(-1, 100_000))
            elif kind == 5:
                ql, rl = -int(rng.integers(1, 50)), -int(rng.integers(1, 50))  # both negative, and so is the length
            a["rb"], a["re"], a["qb"], a["qe"] = rb, rb + rl, qb, qb + ql
            a["score"] = int(rng.integers(1, 300))
            a["sub_n"] = int(rng.choice([-3, -1, 0, 0, 1, 4, 200, 70_000]))
            a["seedcov"] = int(rng.integers(0, 300))
            if neg_seedcov and rng.random() < 0.02:
                a["seedcov"] = -int(rng.integers(1, 100))
        vecs.append(v)
    return vecs
