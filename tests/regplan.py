"""A Python restatement of what pass B of phase 2 decides without a sequence byte (host/regplan_core.h), written from the reference's
lines and not from that header: bns_pos2rid (bntseq.c:316-330), the test, walk and verdict of bwa_fix_xref2 (bwa.c:184-221), infer_bw
(bwamem.c:884-891), the first band (bwamem.c:1187-1191) and the band of a try (bwa.c:116-125), and one region's tries and tasks.
Integers are Python's (no overflow); a double is converted as x86 does it: truncation, INT32_MIN outside the int range."""
import struct

import numpy as np

INT32_MIN = -(1 << 31)
SMALL_CAP = 24
MD_SLOT = 128


def d2i(x):
    return int(x) if x == x and -2147483649.0 < x < 2147483648.0 else INT32_MIN


def cdiv(x, r):
    """(double)x / r as C computes it: IEEE, with the infinities and NaN for r == 0"""
    if r == 0:
        return float("nan") if x == 0 else (float("inf") if x > 0 else float("-inf"))
    return float(x) / float(r)


def pos2rid(contigs, l_pac, pos_f):
    if pos_f >= l_pac:
        return -1
    left, mid, right = 0, 0, len(contigs)
    while left < right:
        mid = (left + right) >> 1
        if pos_f >= contigs[mid][0]:
            if mid == len(contigs) - 1 or pos_f < contigs[mid + 1][0]:
                break
            left = mid + 1
        else:
            right = mid
    return mid


def xref_test(contigs, l_pac, rb, re):
    """-> (verdict, cb, ce): -1 strand bridge, 0 inside its sequence, 1 to be cut to [cb, ce)"""
    if rb < l_pac < re:
        return -1, 0, 0
    fm = (rb + re) >> 1
    is_rev = fm >= l_pac
    if is_rev:
        fm = (l_pac << 1) - 1 - fm
    off, ln = contigs[pos2rid(contigs, l_pac, fm)]
    cb = (l_pac << 1) - (off + ln) if is_rev else off
    ce = cb + ln
    if not (cb > rb or ce < re):
        return 0, 0, 0
    return 1, max(cb, rb), min(ce, re)


def xref_cut(cigar, cb, ce, qb, qe, rb, re):
    """bwa.c:199-221 -> (verdict, qb, qe, rb, re); which: the branches taken, e.g. {"Mb", "De"}"""
    x, y = rb, qb
    for wd in cigar:
        op, ln = int(wd) & 0xf, int(wd) >> 4
        if op == 0:
            if x <= cb < x + ln:
                qb, rb = y + (cb - x), cb
            if x < ce <= x + ln:
                qe, re = y + (ce - x), ce
                break
            x, y = x + ln, y + ln
        elif op == 1:
            y += ln
        elif op == 2:
            if x <= cb < x + ln:
                qb, rb = y, x + ln
            if x < ce <= x + ln:
                qe, re = y, x
                break
            x += ln
    return (-2 if qb == qe or rb == re else 0), qb, qe, rb, re


def cut_branches(cigar, cb, ce, rb, re):
    """which operation holds each cut point that moves an end: a set out of Mb, Db (cb > rb), Me, De (ce < re)"""
    x, out = rb, set()
    for wd in cigar:
        op, ln = int(wd) & 0xf, int(wd) >> 4
        if op in (0, 2):
            if x <= cb < x + ln and cb > rb:
                out.add("MD"[op // 2] + "b")
            if x < ce <= x + ln:
                if ce < re:
                    out.add("MD"[op // 2] + "e")
                break
            x += ln
    return out


def infer_bw(l1, l2, score, a, q, r):
    if l1 == l2 and l1 * a - score < (q + r - a) * 2:
        return 0
    w = d2i(cdiv(min(l1, l2) * a - score - q, r) + 2.0)
    return max(w, abs(l1 - l2))


def first_band(o, ql, tl, truesc, reg_w):
    if truesc == INT32_MIN:
        return reg_w
    w2 = max(infer_bw(ql, tl, truesc, o["a"], o["o_ins"], o["e_ins"]), infer_bw(ql, tl, truesc, o["a"], o["o_del"], o["e_del"]))
    if w2 > o["w"]:
        w2 = min(w2, reg_w)
    return w2


def try_band(o, ql, tl, w2):
    max_ins = d2i(cdiv(((ql + 1) >> 1) * o["mat0"] - o["o_ins"], o["e_ins"]) + 1.0)
    max_del = d2i(cdiv(((ql + 1) >> 1) * o["mat0"] - o["o_del"], o["e_del"]) + 1.0)
    max_gap = max(max_ins, max_del, 1)
    w = min((max_gap + abs(tl - ql) + 1) >> 1, w2)
    return max(w, abs(tl - ql) + 3)


def plan(o, ql, tl, truesc, reg_w):
    """-> (w2, band[3], slot[3], n_tasks, cap)"""
    w2 = first_band(o, ql, tl, truesc, reg_w)
    band, slot, n_tasks, prev = [-1] * 3, [-1] * 3, 0, -1
    cap = min(ql + tl + 2, SMALL_CAP)
    if not (ql == tl and w2 == 0):
        for t in range(1 if truesc == INT32_MIN else 3):
            w = try_band(o, ql, tl, min(w2 << t, (1 << 31) - 1) if w2 >= 0 else w2)
            band[t] = w
            if w == prev:
                slot[t] = slot[t - 1]
                continue
            prev, slot[t] = w, n_tasks
            n_tasks += 1
    return w2, band, slot, n_tasks, cap


def emit_hex(band, slot, n_tasks, cap, q_src, rb, o_off, ql, tl, truesc, task0, cig0):
    """bmh_region_req_t and the bmh_glb_task_t records of one region, as hex"""
    req = struct.pack("<QqQiii3i", q_src, rb, o_off, ql, tl, truesc, *[-1 if s < 0 else task0 + s for s in slot])
    tasks = b""
    for m in range(n_tasks):
        t = slot.index(m)
        tasks += struct.pack("<QQHHiII", o_off, o_off + ql, ql, tl, band[t], cig0 + m * cap, cap)
    return req.hex(), tasks.hex()


def opt_of(p, w=None):
    """the scoring fields the bands read, from a PARAMS record"""
    g = lambda k: int(np.asarray(p[k]).reshape(-1)[0])
    return {"a": g("a"), "mat0": g("mat"), "o_del": g("o_del"), "e_del": g("e_del"), "o_ins": g("o_ins"), "e_ins": g("e_ins"), "w": g("w") if w is None else w}
