"""The band a ksw_extend2 flank needs for its six outputs, restated in Python independently of
host/extband_core.h: the conditions are tried for every w' from 0 up, as they are written down, with no closed form.

    A = max(mat); P(p) = h0 + sum_{k<=p} s(t[k], q[k]) over the plain diagonal, P(-1) = h0; pen_total = A qlen - (P(qlen-1) - h0)
    G(w') = min(o_ins + e_ins (w'+1), o_del + e_del (w'+1));  T(w') = max(o_ins + e_ins w', o_del + e_del w'), T(0) = 0
    w_eff = the smallest w' in [0, w) with  G(w') > pen_total,  h0 >= G(w'),  min_p P(p) > T(w'),
            and zdrop <= 0 or pen_total + max(o_ins + e_ins (w'+1), o_del + e_del (w'+1)) <= zdrop;  else w.
    Left alone (w_eff = w): A < 0, a negative gap cost, qlen < 1 or tlen < qlen.

w_eff(p, pool, tasks) -> int64 per task.  expected_bands(...) -> the byte bmh_last_extend_bands reports per task: w_eff for the
tasks a lane kernel takes (1 <= qlen <= min(128, qmax)), the task's own w for the others and with the narrowing off; 255 stands
for 255 or more."""
import numpy as np

import kswlib


def rule_applies(p):
    return int(np.max(p["mat"])) >= 0 and all(int(p[k]) >= 0 for k in ("o_del", "e_del", "o_ins", "e_ins"))


def one(p, q, t, h0, w):
    """w_eff of one flank: q, t as base codes in flank order"""
    mat = np.asarray(p["mat"], dtype=np.int64).reshape(5, 5)
    o_del, e_del, o_ins, e_ins, zdrop = (int(p[k]) for k in ("o_del", "e_del", "o_ins", "e_ins", "zdrop"))
    qlen, tlen, w = len(q), len(t), int(w)
    if not rule_applies(p) or qlen < 1 or tlen < qlen:
        return w
    A = int(mat.max())
    h0 = max(int(h0), 0)
    s = mat[np.minimum(t[:qlen], 4), np.minimum(q, 4)]
    P = h0 + np.concatenate([[0], np.cumsum(s)])
    pen_total = A * qlen - int(s.sum())
    for wp in range(max(w, 0)):
        gi, gd = o_ins + e_ins * (wp + 1), o_del + e_del * (wp + 1)
        T = max(o_ins + e_ins * wp, o_del + e_del * wp) if wp >= 1 else 0
        if min(gi, gd) > pen_total and h0 >= min(gi, gd) and int(P.min()) > T and (zdrop <= 0 or pen_total + max(gi, gd) <= zdrop):
            return wp
    return w


def w_eff(p, pool, tasks):
    out = np.zeros(len(tasks), np.int64)
    for k, t in enumerate(tasks):
        q, tg = kswlib.task_seqs(pool, t)
        out[k] = one(p, q, tg, t["h0"], t["w"])
    return out


def expected_bands(p, pool, tasks, narrow=True, qmax=128):
    w = tasks["w"].astype(np.int64)
    we = w_eff(p, pool, tasks) if narrow else w
    lane = (tasks["qlen"] >= 1) & (tasks["qlen"] <= min(128, qmax))
    b = np.where(lane, we, w)
    return np.where((b < 0) | (b > 254), 255, b).astype(np.uint8)
