"""Generators and the dispatcher model for ksw_global2 tasks past the wave kernel's LDS row (bin 4, the band ring of
global_kernel.hip): regions of 10 177-65 535 query columns at bands from 1 to a few thousand."""
import numpy as np

import domaingen as dg
import kswgen
import kswlib

# global_kernel's LDS row: H and E int32 [qcap+2], profile 8 bytes [qcap], smat 32 bytes, within 160 KiB (bmh_ctx.h)
LDS_BYTES = 160 * 1024


def _state_bytes(qcap):
    return 8 * (qcap + 2) + 8 * qcap + 32


GLB_LDS_QCAP = max(q for q in range(64, 65536 + 64, 64) if _state_bytes(q) <= LDS_BYTES)  # kGlbLdsQcap
RING_MAX = max(r for r in (1 << k for k in range(6, 17)) if 10 * r + 32 <= LDS_BYTES)     # kGlbRingMax: 10 bytes per slot
MAX_RING_W = (RING_MAX - 2) // 2  # the widest band min(w, qlen) bin 4 takes


def ring_fits(qlen, w):
    return 2 * min(int(w), int(qlen)) + 2 <= RING_MAX


def route(p, tasks, lane_ok=True, long_bin=None):
    """Bin of every task as glb_sort_hist_kernel gives it: 0/3/1 the lane kernels, 2 the wave kernel, 4 the band ring.
    long_bin: whether the launch has a bin 4 -- for host-buffer calls, whenever a task has more than GLB_LDS_QCAP columns."""
    tasks = np.asarray(tasks)
    if len(tasks) == 0:
        return np.zeros(0, np.int32)
    if long_bin is None:
        long_bin = bool((tasks["qlen"] > GLB_LDS_QCAP).any())
    rows_cap = min(max(1, int(tasks["tlen"].max())), 512)
    out = np.empty(len(tasks), np.int32)
    for k, t in enumerate(tasks):
        ql, tl, w = int(t["qlen"]), int(t["tlen"]), int(t["w"])
        b = dg.glb_lane_bin(p, ql, tl, w, rows_cap) if lane_ok else 2
        out[k] = 4 if b == 2 and long_bin and ql > GLB_LDS_QCAP else b
    return out


def long_count(p, tasks, lane_ok=True):
    return int((route(p, tasks, lane_ok) == 4).sum())


def bin2_lds(tasks):
    """The batch-level choice of global_kernel's variant for bin 2 (direction bytes in LDS or HBM), from the maxima of the
    tasks that fit its LDS row; equal to domaingen.glb_wave_lds for a batch without longer tasks."""
    tasks = np.asarray(tasks)
    short = tasks[tasks["qlen"] <= GLB_LDS_QCAP]
    if len(short) == 0:
        short = np.zeros(1, tasks.dtype)
        short["qlen"], short["tlen"], short["w"] = 1, 1, 0
    return dg.glb_wave_lds(short)


def long_pair(rng, qlen, sub=0.01, indel=0.002, max_indel=3, rev=False):
    """A query of qlen bases and the target it came from (substitutions and short indels both ways); rev: both as the reverse
    complement, the way bwa_gen_cigar2 hands over a region on the reverse strand."""
    q = kswgen.rand_seq(rng, qlen)
    t = kswgen.mutate(rng, q, sub, indel, indel, max_indel) if indel or sub else q.copy()
    t = np.asarray(t, np.uint8)
    if rev:
        q, t = (3 - q[::-1]).astype(np.uint8), (3 - t[::-1]).astype(np.uint8)
    return q[:65535], t[:65535]


def gen_long(rng, specs):
    """One ksw_global2 task per (qlen, w, kind) of `specs`.  kind: "cigar" (w raised to |qlen-tlen| where it is smaller, so
    that the band reaches the end cell), "tight" (w = |qlen-tlen|+3, bwa_gen_cigar2's least band), "score" (score only), "short"
    (score only, the target cut so that qlen > tlen + w: the band of the last row ends before qlen).  w = 1 takes
    substitutions only.  Returns (pool, tasks, cigar words)."""
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for qlen, w, kind in specs:
        rev = bool(rng.random() < 0.5)
        if w <= 1:
            q, t = long_pair(rng, qlen, 0.01, 0.0, 1, rev)
        else:
            q, t = long_pair(rng, qlen, 0.01, 0.002, 3, rev)
        if kind == "short":
            t = t[: max(1, len(q) - int(w) - 1 - int(rng.integers(0, 200)))]
        d = abs(len(q) - len(t))
        if kind == "tight":
            w = d + 3
        elif kind == "cigar":
            w = max(int(w), d)
        kswgen._add_glb(pb, q, t, int(w), kind in ("cigar", "tight"))
    return kswgen.finish_glb(pb)


def concat(*batches):
    """Concatenate (pool, tasks, words) batches into one, offsets moved along."""
    pools, tasks, off, words = [], [], 0, 0
    for pool, t, w in batches:
        t = t.copy()
        t["q_off"] += off
        t["t_off"] += off
        t["cigar_off"] += words
        pools.append(pool), tasks.append(t)
        off += len(pool)
        words += int(w)
    return np.concatenate(pools), np.concatenate(tasks), words


def check_against(want, wcig, res, cig, tasks):
    """Score, n_cigar and CIGAR words of a device run against an oracle/reference run; returns the indices that differ."""
    bad = []
    for k, t in enumerate(tasks):
        o, n = int(t["cigar_off"]), int(res[k]["n_cigar"])
        if res[k] != want[k] or (int(t["cigar_cap"]) and not np.array_equal(cig[o:o + n], wcig[k])):
            bad.append(k)
    return bad
