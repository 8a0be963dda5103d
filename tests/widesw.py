"""Generators of the wide Smith-Waterman tests (test_wide_sw_*.py): word-mode ksw_align2 tasks shaped like mem_matesw's
(reference bwamem_pair.c:109-175) whose scores reach the 16-bit clamp, or whose queries run to many kilobases."""
import numpy as np

from kswgen import PoolBuilder, mutate, rand_seq
from kswlib import BMH_F_QCOMP, BMH_F_QREV, BMH_F_TPAC, BMH_F_TREV, KSW_XSTART, KSW_XSUBO, SW_TASK

LDS_COLS = 4096  # == kSwLongLdsCols (csrc/sw_long.hip): longer padded queries run on the slab variant


def matesw_xtra(p, min_seed_len=19):
    """Word-mode xtra as mem_matesw builds it for a long mate (bwamem_pair.c:147): KSW_XSUBO | KSW_XSTART | min_seed_len*a."""
    return KSW_XSUBO | KSW_XSTART | (min_seed_len * int(p["a"]))


def goes_long(p, qlen):
    """Past what the default context accepts: qlen*max(mat) >= 32000."""
    return qlen * int(np.max(p["mat"])) >= 32000


def rescue_pair(rng, qlen, flank, sub=0.01, indel=0.002, hit=True, second=False):
    """(mate, window): the window holds a mutated copy of the mate between random flanks (or none), and sometimes a weaker one."""
    core = rand_seq(rng, qlen)
    tail = int(rng.integers(flank // 2, flank + 1))
    lead = int(rng.integers(0, flank + 1))
    if hit:
        cp = mutate(rng, core, sub=sub, ins=indel, dele=indel, max_indel=3)
        t = np.concatenate([rand_seq(rng, lead), cp, rand_seq(rng, tail)])
        if second:
            weak = mutate(rng, core[: qlen // 3], sub=0.05)
            t = np.concatenate([t, rand_seq(rng, 50), weak])
    else:
        t = rand_seq(rng, lead + qlen + tail)
    return core, t


def add_task(pb, rng, q, t, xtra, flags_ok=True):
    """Store q / t, reversed or complemented at random with the flags that undo it."""
    qrev = flags_ok and rng.random() < 0.4
    qcomp = flags_ok and rng.random() < 0.4
    trev = flags_ok and rng.random() < 0.2
    qs = np.where(q < 4, 3 - q, 4).astype(np.uint8) if qcomp else q
    qo, to = pb.put(qs, qrev), pb.put(t, trev)
    flags = (BMH_F_QREV if qrev else 0) | (BMH_F_TREV if trev else 0) | (BMH_F_QCOMP if qcomp else 0)
    pb.tasks.append((qo, to, len(t), len(q), flags, xtra, 0))


def gen_saturating(rng, p, n, qlen=(300, 700), flank=300, xtra=None):
    """Short word-mode tasks under a large match score: many cells of the copy's diagonal reach 32 767."""
    pb = PoolBuilder(SW_TASK)
    for k in range(n):
        L = int(rng.integers(qlen[0], qlen[1] + 1))
        q, t = rescue_pair(rng, L, flank, sub=0.01 if k % 3 else 0.0, hit=k % 5 != 4, second=k % 4 == 1)
        add_task(pb, rng, q, t, matesw_xtra(p) if xtra is None else xtra)
    return pb.finish()


def gen_tandem(rng, p, n, qlen=(400, 700), period=(3, 12)):
    """A tandem repeat against a window holding more of it: under a large match score whole sets of columns of one row reach
    the clamp together, so qe is decided by the smallest-column rule and the second pass stops on a tie."""
    pb = PoolBuilder(SW_TASK)
    for _ in range(n):
        u = rand_seq(rng, int(rng.integers(period[0], period[1] + 1)))
        L = int(rng.integers(qlen[0], qlen[1] + 1))
        rep = np.tile(u, (3 * L) // len(u) + 2)
        q = rep[:L]
        lead = int(rng.integers(0, 200))
        t = np.concatenate([rand_seq(rng, lead), rep[: L + int(rng.integers(0, L))], rand_seq(rng, 100)])
        add_task(pb, rng, q, t, matesw_xtra(p))
    return pb.finish()


def gen_rescue(rng, p, specs, flank=1500, sub=0.01):
    """One task per (qlen, hit) of specs: a mate against a rescue window, random flags."""
    pb = PoolBuilder(SW_TASK)
    for L, hit in specs:
        q, t = rescue_pair(rng, L, flank, sub=sub, hit=hit, second=rng.random() < 0.3)
        add_task(pb, rng, q, t, matesw_xtra(p))
    return pb.finish()


def gen_rescue_tpac(rng, p, genome_len, specs, flank=1000, sub=0.01):
    """Mates against windows of a 2-bit reference (BMH_F_TPAC on bwa's doubled coordinate, both strands): returns
    (pool, tasks, pac, l_pac).  The pool holds only the mates."""
    g = rand_seq(rng, genome_len)
    pac = np.zeros((genome_len + 3) // 4, dtype=np.uint8)
    for i in range(genome_len):
        pac[i >> 2] |= int(g[i]) << ((~i & 3) << 1)
    pb = PoolBuilder(SW_TASK)
    l_pac = genome_len
    for L, rev_strand in specs:
        W = L + 2 * flank
        st = int(rng.integers(0, genome_len - W))
        win = g[st: st + W]
        if rev_strand:  # the window on the reverse strand: positions 2*l_pac-1-x
            win = (3 - win[::-1]).astype(np.uint8)
            t_off = 2 * l_pac - 1 - (st + W - 1)
        else:
            t_off = st
        src = win[flank: flank + L]
        q = mutate(rng, src, sub=sub, ins=0.002, dele=0.002, max_indel=3)[:L]
        qcomp = rng.random() < 0.5
        qrev = rng.random() < 0.5
        qs = np.where(q < 4, 3 - q, 4).astype(np.uint8) if qcomp else q
        qo = pb.put(qs, qrev)
        flags = BMH_F_TPAC | (BMH_F_QREV if qrev else 0) | (BMH_F_QCOMP if qcomp else 0)
        pb.tasks.append((qo, t_off, W, len(q), flags, matesw_xtra(p), 0))
    pool, tasks = pb.finish()
    return pool, tasks, pac, l_pac


def concat(*batches):
    """Join (pool, tasks) batches into one pool, shifting offsets."""
    pools, tasks, base = [], [], 0
    for pool, t in batches:
        t = t.copy()
        t["q_off"] += base
        tp = (t["flags"] & BMH_F_TPAC) != 0
        t["t_off"] = np.where(tp, t["t_off"], t["t_off"] + base)
        pools.append(pool)
        tasks.append(t)
        base += len(pool)
    return np.concatenate(pools), np.concatenate(tasks)


def sw_shift(p):
    """DevParams.sw_shift: ksw_qinit's byte-mode bias, (uint8_t)(256 - min(mat)) (reference ksw.c:78-85)."""
    return (256 - int(np.min(p["mat"]))) & 0xff


def long_count(p, tasks, wave_cols=320):
    """Tasks a launch sends to the long-query kernel with the switch on (sw_long_takes): word mode, not what sw_wave_kernel takes
    at wave_cols columns (launch_sw: 320 for a batch past 32 768 tasks or with queries past 320 columns, targets up to 16 384)."""
    mx, sh = int(np.max(p["mat"])), sw_shift(p)
    n = 0
    for t in tasks:
        ql, word = int(t["qlen"]), not (int(t["xtra"]) & 0x10000)
        wave = wave_cols > 0 and (ql + 7) // 8 * 8 <= wave_cols and ql * mx + sh < 512
        n += ql >= 1 and word and not wave
    return n


def unseedable(rng, seq, step=18):
    """A copy of seq with a substitution at least every `step` bases: no exact match of step+1 bases survives, so a 19-mer seed
    finds nothing and only mate rescue (ksw_align2) can place the read."""
    out = np.array(seq, dtype=np.uint8).copy()
    for k in range(int(rng.integers(0, step)), len(out), step):
        out[k] = (int(out[k]) + int(rng.integers(1, 4))) & 3
    return out


def long_pairs(rng, genome, n, mate_len, frag_len, n_rescue, sub=0.005):
    """n read pairs (FR: mate 2 is the reverse complement of the fragment's end) with mates of mate_len bases on fragments of
    frag_len bases; the second mate of the last n_rescue pairs is unseedable."""
    r1, r2 = [], []
    for k in range(n):
        L1, L2 = (int(rng.integers(mate_len[0], mate_len[1] + 1)) for _ in range(2))
        F = int(rng.integers(max(frag_len[0], L1, L2), frag_len[1] + 1))
        pos = int(rng.integers(0, len(genome) - F - 1))
        frag = genome[pos: pos + F]
        a = mutate(rng, frag[:L1], sub=sub, ins=0.001, dele=0.001, max_indel=2)
        b = mutate(rng, frag[F - L2:], sub=sub, ins=0.001, dele=0.001, max_indel=2)
        if k >= n - n_rescue:
            b = unseedable(rng, b)
        r1.append(a)
        r2.append((3 - b[::-1]).astype(np.uint8))
    return r1, r2
