"""What the global path's band pass (glb_band_kernel) must return, said in plain Python and without the C header
(host/glbband_core.h): the rule w_eff, the lane kernels' domain, and from the two the byte bmh_last_global_bands reports per task.
Also the small task sets and scorings that the CPU and the GPU tests of the rule share."""
import itertools

import numpy as np

import kswgen
import kswlib

ROWS_CAP = 512  # the lane kernels' direction slab holds this many rows at the most (launch_global)

# the scorings of the exhaustive sets, as arguments of kswlib.make_params
SCORINGS = {
    "default": dict(),
    "asymmetric": dict(o_del=6, e_del=1, o_ins=4, e_ins=2),
    "scaled": dict(a=2, b=8, o_del=12, e_del=2, o_ins=12, e_ins=2),
    "open0": dict(o_del=0, o_ins=0),
    "tie-heavy": dict(a=1, b=1, o_del=0, e_del=1, o_ins=0, e_ins=1),
    "e0": dict(o_del=3, e_del=0, o_ins=2, e_ins=0),
}


def w_eff(p, q, t, w):
    """The rule of host/glbband_core.h, restated (slowly)."""
    mat = np.asarray(p["mat"], dtype=np.int64).reshape(5, 5)
    od, ed, oi, ei = (int(p[k]) for k in ("o_del", "e_del", "o_ins", "e_ins"))
    ql, tl, A = len(q), len(t), int(mat.max())
    d = ql - tl
    if w < abs(d) or ql < 1 or tl < 1 or A <= 0 or min(od, ed, oi, ei) < 0:
        return w
    q, t = np.minimum(q, 4).astype(np.int64), np.minimum(t, 4).astype(np.int64)
    if d == 0:
        lb = int(mat[t, q].sum())
    elif d > 0:
        s0, s1 = mat[t, q[:tl]], mat[t, q[d:]]
        lb = int(s1.sum()) + max(0, int(np.cumsum(s0 - s1).max())) - (oi + ei * d)
    else:
        s0, s1 = mat[t[:ql], q], mat[t[-d:], q]
        lb = int(s1.sum()) + max(0, int(np.cumsum(s0 - s1).max())) - (od + ed * -d)
    K = A + ei + ed
    xp, xm = A * ql - oi - od + ed * d - lb, A * tl - oi - od - ei * d - lb
    return min(w, max(abs(d), xp // K if xp >= 0 else 0, xm // K if xm >= 0 else 0))


def lane_domain(p, ql, tl, w, rows_cap):
    """May a lane-per-task kernel take the task (glb_lane_domain): its rows fit the slab and no cell can leave 16 bits."""
    mat = np.asarray(p["mat"], dtype=np.int64)
    od, ed, oi, ei = (int(p[k]) for k in ("o_del", "e_del", "o_ins", "e_ins"))
    smax = max(int(-mat.min()), int(max(mat.max(), 0)))
    worst = od + oi + max(ed, ei) * (ql + tl) + smax * max(ql, tl)
    return tl <= rows_cap and worst < 12000 and od + oi < 4000 and w >= 0


def lane_domain_all(p, tasks, rows_cap):
    """lane_domain of every task of a batch at once."""
    mat = np.asarray(p["mat"], dtype=np.int64)
    od, ed, oi, ei = (int(p[k]) for k in ("o_del", "e_del", "o_ins", "e_ins"))
    smax = max(int(-mat.min()), int(max(mat.max(), 0)))
    ql, tl = tasks["qlen"].astype(np.int64), tasks["tlen"].astype(np.int64)
    worst = od + oi + max(ed, ei) * (ql + tl) + smax * np.maximum(ql, tl)
    return (tl <= rows_cap) & (worst < 12000) & (od + oi < 4000) & (tasks["w"].astype(np.int64) >= 0)


def expected_bands(p, pool, tasks, rows_cap=None):
    """The byte of every task, in the order given: the rule's band where the rule and the lane kernels' domain apply, else the task's
    own w; 255 for everything past a byte.  rows_cap: of a host-fed batch (the default) the longest target, up to ROWS_CAP."""
    if rows_cap is None:
        rows_cap = min(int(tasks["tlen"].max()), ROWS_CAP) if len(tasks) else ROWS_CAP
    out = np.zeros(len(tasks), dtype=np.uint8)
    dom = lane_domain_all(p, tasks, rows_cap)
    for k, x in enumerate(tasks):
        ql, tl, w = int(x["qlen"]), int(x["tlen"]), int(x["w"])
        if dom[k]:
            qo, to = int(x["q_off"]), int(x["t_off"])
            w = w_eff(p, pool[qo:qo + ql], pool[to:to + tl], w)
        out[k] = 255 if w < 0 or w > 255 else w
    return out


def exhaustive_set(letters, maxlen, wmax):
    """Every (q, t) over the first `letters` base codes with lengths 1..maxlen, at every w from |qlen - tlen| to wmax; all with a CIGAR."""
    seqs = [np.array(s, dtype=np.uint8) for n in range(1, maxlen + 1) for s in itertools.product(range(letters), repeat=n)]
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for q in seqs:
        for t in seqs:
            for w in range(abs(len(q) - len(t)), wmax + 1):
                kswgen._add_glb(pb, q, t, w)
    return kswgen.finish_glb(pb)


def set_a():
    return exhaustive_set(2, 5, 6)  # 22 732 tasks


def set_b():
    return exhaustive_set(3, 3, 4)  # 6 741 tasks
