"""Word-mode ksw_align2 (reference bwa-0.7.8/ksw.c:231-364) restated column-parallel in numpy, with the one place the 16-bit
lanes of ksw_i16 change a result: the saturating add H(i-1,j-1) + S, which clamps at 32 767.  Every other operation of
ksw_i16 stays inside [0, 32767] (subs_epu16 of non-negative operands, signed max of values <= 32767), so H, E and F need no
other clamp.  This is the specification of sw_long_kernel (csrc/sw_long.hip); test_wide_sw_cpu.py pins it to the compiled
reference where scores cross 32 767.

A row, over the query padded to Q = 8*slen columns (pad columns score 0):
  a(j)  = max(min(H(i-1,j-1) + S(t_i, q_j), 32767), E(i,j))
  w(j)  = a(j) - o_ins - e_ins + e_ins*j
  Ffull = max(0, exclusive prefix max of w - e_ins*(j-1))        the lazy-F pass, ksw.c:278-288
  Fseg  = the same prefix restricted to j's segment [k*slen, (k+1)*slen)   the main loop's f, ksw.c:262-276
  Hpre = max(a, Fseg),  H = max(Hpre, Ffull),  E' = max(0, E - e_del, Hpre - o_del - e_del)
"""
import numpy as np

from kswlib import KSW_XSTART, KSW_XSTOP, KSW_XSUBO, SW_RES, SW_FIELDS, sw_task_seqs

SAT = 32767
NEG = -(1 << 40)


def _excl_prefix_max(w):
    """Exclusive prefix maximum along the last axis (NEG where nothing precedes)."""
    inc = np.maximum.accumulate(w, axis=-1)
    out = np.empty_like(inc)
    out[..., 0] = NEG
    out[..., 1:] = inc[..., :-1]
    return out


def sw_pass(q, t, mat, max_mat, o_del, e_del, o_ins, e_ins, minsc, endsc, stats=None):
    """One call of ksw_i16; returns (score, te, qe, score2, te2).  stats (a dict), if given, receives the number of columns
    of the saved row that hold the maximum ("qe_ties")."""
    qlen = len(q)
    slen = (qlen + 7) // 8
    Q = 8 * slen
    if slen == 0:
        return 0, -1, 0, -1, -1
    m = np.asarray(mat, dtype=np.int64).reshape(5, 5)
    code = np.full(Q, 5, dtype=np.int64)
    code[:qlen] = np.minimum(np.asarray(q, dtype=np.int64), 4)
    prof = np.zeros((5, 6), dtype=np.int64)  # [target base][query code], code 5 = pad
    prof[:, :5] = m
    j = np.arange(Q, dtype=np.int64)
    wadd = e_ins * j - o_ins - e_ins
    fsub = e_ins * (j - 1)
    H = np.zeros(Q, dtype=np.int64)
    E = np.zeros(Q, dtype=np.int64)
    Hmax = np.zeros(Q, dtype=np.int64)
    gmax, te = 0, -1
    b = []  # [score, row] entries, ksw.c:290-300
    tt = np.minimum(np.asarray(t, dtype=np.int64), 4)
    for i in range(len(t)):
        diag = np.empty(Q, dtype=np.int64)
        diag[0] = 0
        diag[1:] = H[:-1]
        a = np.maximum(np.minimum(diag + prof[tt[i]][code], SAT), E)
        w = a + wadd
        ffull = np.maximum(_excl_prefix_max(w) - fsub, 0)
        fseg = np.maximum(_excl_prefix_max(w.reshape(8, slen)).reshape(Q) - fsub, 0)
        hpre = np.maximum(a, fseg)
        H = np.maximum(hpre, ffull)
        E = np.maximum(np.maximum(E - e_del, hpre - o_del - e_del), 0)
        imax = int(H.max())
        if imax >= minsc:
            if not b or b[-1][1] + 1 != i:
                b.append([imax, i])
            elif b[-1][0] < imax:
                b[-1] = [imax, i]
        if imax > gmax:
            gmax, te = imax, i
            Hmax = H.copy()
            if gmax >= endsc:
                break
    qe = int(np.argmax(Hmax))  # smallest column of the maximum, ksw.c:316-320 (all zero: column 0)
    if stats is not None:
        stats["qe_ties"] = int((Hmax == Hmax[qe]).sum())
    score2, te2 = -1, -1
    if b:
        d = (gmax + max_mat - 1) // max_mat
        for sc, row in b:
            if (row < te - d or row > te + d) and sc > score2:
                score2, te2 = sc, row
    return gmax, te, qe, score2, te2


def align2(q, t, p, xtra):
    """ksw_align2 in word mode (xtra without KSW_XBYTE); returns a dict of the kswr_t fields."""
    mat = np.asarray(p["mat"], dtype=np.int64)
    mx = int(mat.max())
    o_del, e_del, o_ins, e_ins = int(p["o_del"]), int(p["e_del"]), int(p["o_ins"]), int(p["e_ins"])
    thr = xtra & 0xffff
    minsc = thr if xtra & KSW_XSUBO else 0x10000
    endsc = thr if xtra & KSW_XSTOP else 0x10000
    score, te, qe, score2, te2 = sw_pass(q, t, mat, mx, o_del, e_del, o_ins, e_ins, minsc, endsc)
    r = dict(score=score, te=te, qe=qe, score2=score2, te2=te2, tb=-1, qb=-1)
    if not (xtra & KSW_XSTART) or ((xtra & KSW_XSUBO) and score < thr):
        return r
    q2 = np.asarray(q)[: qe + 1][::-1]
    t2 = np.asarray(t).copy()
    t2[: te + 1] = t2[: te + 1][::-1]
    rs, rte, rqe, _, _ = sw_pass(q2, t2, mat, mx, o_del, e_del, o_ins, e_ins, 0x10000, score)
    if rs == score:
        r["tb"], r["qb"] = te - rte, qe - rqe
    return r


def sat_sw_batch(p, pool, tasks, pac=None, l_pac=0):
    """align2 over SW_TASK records (word mode only)."""
    out = np.zeros(len(tasks), dtype=SW_RES)
    for k, tk in enumerate(tasks):
        assert not (int(tk["xtra"]) & 0x10000), "word mode only"
        q, tg = sw_task_seqs(pool, tk, pac, l_pac)
        r = align2(q, tg, p, int(tk["xtra"]))
        out[k] = tuple(r[f] for f in SW_FIELDS) + (0,)
    return out
