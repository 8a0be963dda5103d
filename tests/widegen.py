"""Generators and dispatcher conditions for the int32 extension kernel (extend_wide.hip, bmh_ctx_set_wide_extension): tasks past
the 16-bit score range, past the LDS kernel's query capacity and under gap costs past 16 bits."""
import numpy as np

import domaingen as dg
import kswgen
import kswlib

LDS_QCAP = 13632       # kLdsQcap, bwa-mem-quickassist_amd/csrc/bmh_ctx.h: the longest query of extend_lds_kernel
WIDE_LDS_QCAP = 12544  # kWideLdsQcap: the longest query the wide kernel keeps in LDS; longer ones use its HBM slab
WIDE_LIMIT = 1 << 24   # kWideScoreLimit, bmh_device.h: h0 + qlen*max(mat) the wide kernel accepts


def goes_wide(p, qlen, h0):
    """ext_goes_wide + the batch-wide gap rule of launch_extend (extend_dispatch.hip), for a context with the switch on."""
    if not dg.ext_gaps_accepted(p):
        return True
    return max(int(h0), 0) + int(qlen) * dg.max_mat(p) > dg.LIMIT or int(qlen) > LDS_QCAP


def wide_count(p, tasks):
    return sum(goes_wide(p, int(t["qlen"]), int(t["h0"])) for t in tasks)


def gen_ext(rng, p, specs, w=(20, 60, 150), sub=0.01, indel=0.003, tgap=60):
    """One extension task per (qlen, h0) in `specs`: a target that starts with a mutated copy of the query, bands from `w`,
    end bonuses 0 or 5, query and target stored forwards or reversed at random."""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for qlen, h0 in specs:
        q, t = dg.related(rng, qlen, min(65535, qlen + tgap), sub=sub, indel=indel, max_indel=2)
        kswgen._add_ext(pb, rng, q, t, int(h0), int(rng.choice(w)), int(rng.choice([0, 5])))
    return pb.finish()


def gen_mixed(rng, p, n_in=48, n_wide=8, wide_q=(3000, 4000), w=(20, 60)):
    """A batch in which most tasks sit inside the 16-bit domain (every length bin) and some just above it."""
    mx = dg.max_mat(p)
    specs = []
    for k in range(n_in):
        q = int(rng.choice([20, 50, 100, 200, 400, 900, 2000]))
        q = min(q, (dg.LIMIT - 1) // mx)
        specs.append((q, int(rng.integers(0, dg.LIMIT - q * mx + 1))))
    for k in range(n_wide):
        q = int(rng.integers(*wide_q))
        specs.append((q, max(1000, dg.LIMIT - q * mx + 1 + int(rng.integers(0, 3000)))))  # (h0 = 0 would end the extension at once)
    order = rng.permutation(len(specs))
    return gen_ext(rng, p, [specs[i] for i in order], w=w)


WIDE_GAP_SETS = [  # gap costs ext_gaps_too_large refuses with the switch off
    dict(o_del=6, e_del=16384, o_ins=6, e_ins=16384),
    dict(o_del=0, e_del=25535, o_ins=0, e_ins=25535),
    dict(o_del=0, e_del=65535, o_ins=0, e_ins=65535),
    dict(o_del=69999, e_del=1, o_ins=69999, e_ins=1),
    dict(o_del=4465, e_del=65535, o_ins=6, e_ins=1),
]


def long_reads(rng, genome, n, lens, sub=0.01, indel=0.002):
    """n reads sampled from `genome` (codes 0-3) with lengths drawn from `lens` = (lo, hi), half of them reverse-complemented."""
    out = []
    for _ in range(n):
        L = int(rng.integers(lens[0], lens[1] + 1))
        s = int(rng.integers(0, len(genome) - L))
        r = kswgen.mutate(rng, genome[s:s + L], sub, indel, indel, 2)
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        out.append(np.ascontiguousarray(r, dtype=np.uint8))
    return out


def gen_seeds(rng, L, n, indel=0.0, qbegs=()):
    """n seed records on reads of about L bases, each read a mutated copy (substitutions, and indels of up to 3 bases at rate
    `indel`) of the middle of its window; `qbegs` fixes the seed start of the first seeds (their flanks stay as generated)."""
    pool, rows = [], []
    off = 0
    for k in range(n):
        win = kswgen.rand_seq(rng, L + 200)
        read = kswgen.mutate(rng, win[100:100 + L], 0.01, indel, indel, 3).astype(np.uint8)
        lq = len(read)
        ln = int(rng.integers(19, 31))
        qbeg = int(qbegs[k]) if k < len(qbegs) else int(rng.integers(0, lq - ln))
        rbeg = min(100 + qbeg, L + 200 - ln)
        pool += [read, win]
        rows.append((off, off + lq, lq, qbeg, ln, rbeg, L + 200, 0, 0))
        off += lq + L + 200
    pool.append(np.zeros(16, np.uint8))
    return np.concatenate(pool).astype(np.uint8), np.array(rows, dtype=kswlib.SEED_TASK)
