"""The rows a ksw_extend2 flank runs on the extension lane kernels, restated in Python independently of host/extstop_core.h: the
reference's recurrence (ksw.c:379-476) over all tasks of a batch at once, one numpy vector per DP column, with the early-stop rule of
DESIGN.md §4.3 in the block form the kernels take:

    A = max(mat); the rule applies iff A >= 0 and the four gap costs are >= 0
    after row i (cells, gscore update, max update, loop not broken):
      U = max(first-column value of row i + A * (qlen - beg),
              over the 8-column blocks counted from the query's right end in which the task has a live column:
                  (row maximum over the live columns up to the block's end) + A * (8 r + 7),  r = block number from the right)
      stop iff U <= max and U < gscore

rows(p, pool, tasks, rule=True) -> (rows per task, the six outputs per task as an EXT_RES array).  With rule=False, or a scoring the
rule does not apply to, the rows are the reference's own."""
import numpy as np

import kswlib


def rule_applies(p):
    return int(np.max(p["mat"])) >= 0 and all(int(p[k]) >= 0 for k in ("o_del", "e_del", "o_ins", "e_ins"))


def rows(p, pool, tasks, rule=True):
    n = len(tasks)
    mat = np.asarray(p["mat"], dtype=np.int64)
    o_del, e_del, o_ins, e_ins, zdrop = (int(p[k]) for k in ("o_del", "e_del", "o_ins", "e_ins", "zdrop"))
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    A = int(mat.max())
    rule = rule and rule_applies(p)
    qlen, tlen = tasks["qlen"].astype(np.int64), tasks["tlen"].astype(np.int64)
    Q, T = int(qlen.max()), int(tlen.max())
    qs, ts = np.full((n, Q + 1), 4, np.int64), np.full((n, T + 1), 4, np.int64)
    for k, t in enumerate(tasks):
        q, tg = kswlib.task_seqs(pool, t)
        qs[k, :len(q)], ts[k, :len(tg)] = np.minimum(q, 4), np.minimum(tg, 4)
    h0 = np.maximum(tasks["h0"].astype(np.int64), 0)
    cols = np.arange(Q + 2)[None, :]
    H, E = np.zeros((n, Q + 2), np.int64), np.zeros((n, Q + 2), np.int64)
    H[:, 0] = h0
    H[:, 1] = np.where(h0 > oe_ins, h0 - oe_ins, 0)
    for j in range(2, Q + 1):
        H[:, j] = np.where((j <= qlen) & (H[:, j - 1] > e_ins), H[:, j - 1] - e_ins, 0)
    mx = max(A, 0)
    eb = tasks["end_bonus"].astype(np.int64)
    w = tasks["w"].astype(np.int64)
    w = np.minimum(w, np.maximum(((qlen * mx + eb - o_ins).astype(np.float64) / e_ins + 1.).astype(np.int64), 1))
    w = np.minimum(w, np.maximum(((qlen * mx + eb - o_del).astype(np.float64) / e_del + 1.).astype(np.int64), 1))
    best, bi, bj = h0.copy(), np.full(n, -1), np.full(n, -1)
    gs, gi, moff = np.full(n, -1), np.full(n, -1), np.zeros(n, np.int64)
    beg, end = np.zeros(n, np.int64), qlen.copy()
    nrows = np.zeros(n, np.int64)
    act = tlen > 0
    ar = np.arange(n)
    i = 0
    while act.any():
        act &= i < tlen
        if not act.any():
            break
        nrows[act] = i + 1
        h1 = np.maximum(h0 - (o_del + e_del * (i + 1)), 0)
        beg = np.where(act, np.maximum(beg, i - w), beg)
        end = np.where(act, np.minimum(np.minimum(end, i + w + 1), qlen), end)
        f, m, mj = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1)
        u = h1 + A * (qlen - beg)
        srow = mat.reshape(5, 5)[ts[:, i]]  # (n, 5): the scores of this row's target base
        lo, hi = (int(beg[act].min()), int(end[act].max()))
        for j in range(lo, hi):
            live = act & (beg <= j) & (j < end)
            if not live.any():
                continue
            h, e = H[:, j], E[:, j]
            hh = np.maximum(np.maximum(h + srow[ar, qs[:, j]], e), f)
            H[:, j] = np.where(live, h1, h)
            h1 = np.where(live, hh, h1)
            mj = np.where(live & (hh >= m), j, mj)
            m = np.where(live, np.maximum(m, hh), m)
            E[:, j] = np.where(live, np.maximum(e - e_del, np.maximum(hh - oe_del, 0)), e)
            f = np.where(live, np.maximum(f - e_ins, np.maximum(hh - oe_ins, 0)), f)
            right = qlen - 1 - j
            at = live & ((right % 8 == 0) | (j == end - 1))
            term = m + A * (right // 8 * 8 + 7)
            u = np.where(at & (term > u), term, u)
        H[ar[act], end[act]] = h1[act]
        E[ar[act], end[act]] = 0
        jfin = np.where(end > beg, end, beg)
        atq = act & (jfin == qlen)
        gi = np.where(atq & (h1 >= gs), i, gi)
        gs = np.where(atq, np.maximum(gs, h1), gs)
        stop = act & (m == 0)
        upd = act & ~stop & (m > best)
        dd = (i - bi) - (mj - bj)
        pen = np.where(dd > 0, dd * e_del, -dd * e_ins)
        stop |= act & ~upd & (zdrop > 0) & (best - m - pen > zdrop)
        moff = np.where(upd, np.maximum(moff, np.abs(mj - i)), moff)
        best, bi, bj = np.where(upd, m, best), np.where(upd, i, bi), np.where(upd, mj, bj)
        if rule:
            stop |= act & (u <= best) & (u < gs)
        act &= ~stop
        zero = H == 0
        cl = zero & (cols >= beg[:, None]) & (cols <= mj[:, None])
        last = np.where(cl.any(1), Q + 1 - np.argmax(cl[:, ::-1], 1), beg - 1)
        cr = zero & (cols >= mj[:, None] + 2) & (cols <= end[:, None])
        first = np.where(cr.any(1), np.argmax(cr, 1), end + 1)
        beg, end = np.where(act, last + 1, beg), np.where(act, first, end)
        i += 1
    out = np.zeros(n, dtype=kswlib.EXT_RES)
    out["score"], out["qle"], out["tle"], out["gtle"], out["gscore"], out["max_off"] = best, bj + 1, bi + 1, gi + 1, gs, moff
    return nrows, out
