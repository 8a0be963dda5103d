"""Hand-made extension tasks around the early-stop rule, shared by its CPU and GPU tests: every kind at a given
query length, so that the GPU test can put them through each instantiation of the lane kernels."""
import numpy as np

import kswgen
import kswlib


def _flip(s):
    return ((np.asarray(s, dtype=np.uint8) + 1) & 3).astype(np.uint8)


def targeted(rng, L, reps=2):
    """(pool, tasks, kind of each task) with queries of exactly L columns (1 <= L) unless the kind says otherwise."""
    pb, kinds = kswgen.PoolBuilder(kswlib.EXT_TASK), []

    def add(kind, q, t, h0, w, eb=5):
        q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
        if len(q) < 1 or len(t) < 1:
            return
        kswgen._add_ext(pb, rng, q, t, int(h0), int(w), int(eb))
        kinds.append(kind)

    for _ in range(reps):
        q = kswgen.rand_seq(rng, L)
        tail = kswgen.rand_seq(rng, L + 40)
        # a late maximum after a long poor stretch: the middle third mismatches, the seed's score carries the flank across it
        t = q.copy()
        a, b = L // 4, max(L // 4 + 1, L // 4 + min(L // 3, 30))
        t[a:b] = _flip(t[a:b])
        add("late_max", q, np.concatenate([t, tail]), 40 + 4 * (b - a), 100)
        add("late_max_lowh0", q, np.concatenate([t, tail]), 5 * (b - a), 100)
        # an equal gscore in a later row: one letter, so that every row that reaches the query's end ties or falls by a gap
        add("gscore_tie", np.zeros(L, np.uint8), np.zeros(2 * L + 8, np.uint8), int(rng.integers(0, 30)), 100)
        rep = np.tile(kswgen.rand_seq(rng, int(rng.integers(1, 4))), L + 8)
        add("gscore_tie_rep", rep[:L], np.concatenate([rep[1:L - 1], rep[:L + 12]]), int(rng.integers(0, 30)), 100)
        # the query's end is never reached: a narrow band and a target too short for it
        add("no_gscore", q, q[:max(1, L - 8)], 30, 3)
        add("no_gscore_band", q, np.concatenate([q[:L // 2], tail]), 30, 2)
        # beg > 0 with a large h0: the band moves beg, and the first-column value is still positive there
        for w in (1, 3, 6):
            add("beg_quirk", q, np.concatenate([kswgen.mutate(rng, q, 0.03, 0.01, 0.01, 2), tail]), int(rng.integers(100, 200)), w)
        # interior zero cells that restart at +A: a low start and bursts of mismatches
        t = q.copy()
        for s in range(6, L, 17):
            t[s:s + 5] = _flip(t[s:s + 5])
        add("restart", q, np.concatenate([t, tail]), int(rng.integers(1, 8)), 100)
        # a perfect flank, a perfect flank behind one insertion, and one behind a deletion: the rule fires a few rows behind the diagonal
        add("perfect", q, np.concatenate([q, tail]), int(rng.integers(19, 100)), 100)
        add("perfect_ins", q, np.concatenate([q[:L // 2], kswgen.rand_seq(rng, 3), q[L // 2:], tail]), 60, 100)
        add("perfect_del", q, np.concatenate([q[:L // 2], q[L // 2 + 2:], tail]), 60, 100)
        # the rule fires at the last row, or one row before or behind it
        for cut in (-1, 0, 1, 2, 5):
            add("last_row", q, np.concatenate([q, tail])[:max(1, L + cut)], 25, 100)
        # N-rich
        qn = kswgen.rand_seq(rng, L, 0.2)
        tn = np.concatenate([np.where(qn > 3, 0, qn).astype(np.uint8), tail])
        tn[rng.random(len(tn)) < 0.1] = 4
        add("n_rich", qn, tn, int(rng.integers(10, 80)), 100)
        # unrelated: m == 0 or z-drop long before any bound
        add("unrelated", q, kswgen.rand_seq(rng, 2 * L + 8), int(rng.integers(0, 40)), 100)
        # garbage behind a good half: z-drop country (the test runs these under several zdrop values)
        add("zdrop", q, np.concatenate([q[:L // 2], kswgen.rand_seq(rng, L + 30)]), 50, 100)
        add("zdrop_gap", q, np.concatenate([q[:L // 2], kswgen.rand_seq(rng, 12), q[L // 2:], tail]), 50, 100)
    pool, tasks = pb.finish()
    return pool, tasks, kinds


def tiny(rng):
    """qlen and tlen of 1 to 3 over two letters and N, several h0."""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for ql in (1, 2, 3):
        for tl in (1, 2, 3, 4):
            for h0 in (0, 1, 7, 30):
                for _ in range(3):
                    kswgen._add_ext(pb, rng, kswgen.rand_seq(rng, ql, 0.1, 2), kswgen.rand_seq(rng, tl, 0.1, 2), h0, int(rng.choice([1, 100])), 5)
    return pb.finish()


def merge(parts):
    """[(pool, tasks)] -> one (pool, tasks) with the offsets moved."""
    pools, tasks, off = [], [], 0
    for pool, t in parts:
        t = t.copy()
        t["q_off"] += off
        t["t_off"] += off
        pools.append(pool)
        tasks.append(t)
        off += len(pool)
    return np.concatenate(pools), np.concatenate(tasks)
