"""Hand-made ksw_extend2 tasks for the band rule of DESIGN.md §4.3 (host/extband_core.h), shared by its CPU and GPU tests.

All of them under bwa's default scoring (a 1, b 4, N -1, o 6, e 1, zdrop 100) unless a test runs them under another one."""
import numpy as np

import kswgen
import kswlib


def _add(pb, q, t, h0, w, eb=5, qrev=False, trev=False):
    qo, to = pb.put(q, qrev), pb.put(t, trev)
    pb.tasks.append((qo, to, len(q), len(t), h0, w, eb, (kswlib.BMH_F_QREV if qrev else 0) | (kswlib.BMH_F_TREV if trev else 0), 0))


TRANSIENT_Q = np.array([2, 3, 1, 0, 3, 1, 3, 2, 3, 2, 2, 0, 1, 0], np.uint8)
TRANSIENT_T = np.concatenate([np.array([2, 3, 1, 3, 2, 1, 3, 2, 3, 2, 2, 0, 1, 0], np.uint8), np.tile(np.array([1, 2, 0], np.uint8), 12)])


def handmade(rng):
    """The two classes that broke earlier forms of the rule: h0 in {0, 1} against good sequences (restarts from zero cells make
    max_off differ under a narrow band), and the transient gscore (a row maximum three columns off the diagonal behind a true zero).
    Returns (pool, tasks, index of the transient task)."""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for k in range(120):
        L = int(rng.integers(3, 90))
        q, t = kswgen.flank_pair(rng, L, int(rng.integers(0, 30)), 0.02 * (k % 3), 0.0, 0.0)
        _add(pb, q, t, k % 2, int(rng.choice([100, 32, 3, 1])), 5, k % 5 == 0, k % 7 == 0)
    at = len(pb.tasks)
    _add(pb, TRANSIENT_Q, TRANSIENT_T, 12, 32, 5)
    for w in (1, 3, 8, 13, 14, 100):  # the same flank at other bands, and with other h0
        _add(pb, TRANSIENT_Q, TRANSIENT_T, 12, w, 5)
        _add(pb, TRANSIENT_Q, TRANSIENT_T, 12 + w % 7, w, 0)
    return pb.finish() + (at,)


def boundary(rng, L=30, w=100):
    """Tasks one unit on either side of each condition of the rule under the default scoring (o + e = 7, a mismatch loses 5, an N 2,
    against a match): (pool, tasks, {name: (index narrowed, its band, index left alone)}).
      1  tlen = qlen against tlen = qlen - 1
      2  pen_total = 6 (three N: G(0) = 7 > 6) against pen_total = 7 ... with pen_total = 8 (four N) the band is 2, not 0:
         reported as the pair (band 0, band 2); and pen_total so large that no band below w qualifies
      3  h0 = 7 = G(0) against h0 = 6
      4  two mismatches in front (the diagonal dips by 8, pen_total = 10, band 4, T(4) = 10): h0 = 19 against h0 = 18
      5  is a property of zdrop: the perfect flank at zdrop = 7 against zdrop = 6 -- the test runs `perfect` under both"""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    q = kswgen.rand_seq(rng, L)
    tail = kswgen.rand_seq(rng, 12)
    full = np.concatenate([q, tail])
    idx = {}

    def add(qq, tt, h0, ww=w):
        _add(pb, qq, tt, h0, ww, 5)
        return len(pb.tasks) - 1

    idx["1"] = (add(q, full[:L], 40), 0, add(q, full[:L - 1], 40))
    n3, n4 = q.copy(), q.copy()
    n3[[5, 11, 17]] = 4
    n4[[5, 11, 17, 23]] = 4
    idx["2"] = (add(n3, full, 40), 0, add(n4, full, 40))  # (the second is narrowed too, to 2: see above)
    many = (q + 1) & 3  # pen_total = 5 L = 150: G(w') > 150 only from w' = 144 on
    idx["2far"] = (add(n4, full, 40), 2, add(many, full, 40))
    idx["3"] = (add(q, full, 7), 0, add(q, full, 6))
    mm = full.copy()
    mm[:2] = (mm[:2] + 1) & 3
    idx["4"] = (add(q, mm, 19), 4, add(q, mm, 18))
    idx["perfect"] = (add(q, full, 40), 0, -1)
    idx["w"] = (add(q, full, 40, 1), 0, add(q, full, 40, 0))  # w = 1 narrows to 0; w = 0 has nothing below it
    return pb.finish() + (idx,)
