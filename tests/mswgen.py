"""Deterministic inputs for the mate-rescue drivers (bmh_matesw_batch, bmh_matesw_device), built in numpy: one genome of 60 kbp with its
2-bit pac, and region vectors written directly -- they need not come from an aligner, the drivers take them as phase 1's output.

Three families of pairs, made to reach what the committed fixture (tests/golden/matesw_golden.npz) does not: vectors of a dozen regions,
dozens of ksw_align2 calls per pair, a second and third round, anchors at the strand ends, and word mode.
  dispersed   a 700-bp unit planted 12 times, 2 500 bp apart.  The anchor is 150 bp from inside the unit with 12 hits whose scores lie
              within pen_unpaired of each other (two of them displaced, so that their windows cut the mate's copy and rescue finds a
              redundant part of it); the mate is the reverse complement of the 150 bp that start 330 bp downstream, lightly mutated.  The mate's vector is empty in half of the pairs and holds hits at a random third of the copies in the rest.
              Either read may be the anchor, on either strand.
  tandem      a 300-bp unit repeated 12 times head to tail.  Anchors of 100 bp with 10 hits 300 bp apart, so the windows overlap and
              the same mate hit is found from several anchors; mates of 100-120 bp; the mate's vector starts empty.
  edge        single-hit anchors of 100 bp at the ends of the two strands, with mates of 80, 130 and 150 bp.
Inactive pairs (proper FR pairs, and pairs without any hit) need no rescue under the FR-only table."""
import functools

import numpy as np

import kswlib

L_PAC = 60000
LOW, HIGH = 13, 678
UNIT_D, N_D, STEP_D, BASE_D = 700, 12, 2500, 2000  # dispersed
UNIT_T, N_T, BASE_T = 300, 12, 34000               # tandem
FREE0, FREE1 = 39000, 58000                        # unique sequence for the inactive pairs

# (pen_unpaired, max_matesw, min_seed_len): mem_opt_init's values first
OPTS = {"default": (17, 100, 19), "one": (17, 1, 19), "three": (17, 3, 19), "best_only": (0, 100, 19)}
TABLES = {"fr": (1, 0, 1, 1), "all": (0, 0, 0, 0), "none": (1, 1, 1, 1)}
LEVEL = 0.95  # mask_level_redun, mem_opt_init


def scoring(name):
    """byte: a=1, b=4 (150 bp x 1 < 250: ksw_u8); word: a=2, b=5, o=8 (150 bp x 2 >= 250: ksw_i16)."""
    return kswlib.make_params() if name == "byte" else kswlib.make_params(a=2, b=5, o_del=8, o_ins=8)


def opt(name):
    o = np.zeros((), dtype=kswlib.MATESW_OPT)
    o["pen_unpaired"], o["max_matesw"], o["min_seed_len"] = OPTS[name]
    return o


def pes(name):
    t = np.zeros(4, dtype=kswlib.PESTAT)
    t["low"], t["high"], t["avg"], t["std"] = LOW, HIGH, 345.5, 60.0
    t["failed"] = TABLES[name]
    return t


@functools.lru_cache(maxsize=None)
def genome():
    """(l_pac, pac, base codes)"""
    rng = np.random.default_rng(20240611)
    ref = rng.integers(0, 4, L_PAC).astype(np.uint8)
    unit = rng.integers(0, 4, UNIT_D).astype(np.uint8)
    for k in range(N_D):
        ref[BASE_D + STEP_D * k: BASE_D + STEP_D * k + UNIT_D] = unit
    ref[BASE_T: BASE_T + UNIT_T * N_T] = np.tile(rng.integers(0, 4, UNIT_T).astype(np.uint8), N_T)
    pad = np.concatenate([ref, np.zeros(-L_PAC % 4, np.uint8)]).reshape(-1, 4)
    pac = (pad[:, 0] << 6 | pad[:, 1] << 4 | pad[:, 2] << 2 | pad[:, 3]).astype(np.uint8)
    ref.setflags(write=False), pac.setflags(write=False)
    return L_PAC, pac, ref


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def _mutate(rng, s, n):
    s = s.copy()
    for k in rng.choice(len(s), n, replace=False):
        s[k] = (s[k] + 1 + rng.integers(0, 3)) & 3
    return s


def _region(rb, length, score, a=1):
    r = np.zeros((), dtype=kswlib.ALNREG)
    r["rb"], r["re"], r["qb"], r["qe"] = rb, rb + length, 0, length
    r["score"] = r["truesc"] = score * a
    r["seedcov"], r["w"] = length >> 1, 100
    r["secondary"] = -1
    return r


def _vector(regs):
    v = np.array(regs, dtype=kswlib.ALNREG).reshape(-1) if regs else np.zeros(0, dtype=kswlib.ALNREG)
    return v[np.argsort(-v["score"], kind="stable")]


def _on_strand(fwd_beg, length, rev):
    """rb of the forward interval [fwd_beg, fwd_beg + length) as a hit of a read on the forward (rev = False) or reverse strand"""
    return 2 * L_PAC - (fwd_beg + length) if rev else fwd_beg


def _oriented(pair, swap):
    (ra, va), (rm, vm) = pair
    return ([rm, ra], [vm, va]) if swap else ([ra, rm], [va, vm])


def dispersed(rng, a, k):
    _, _, ref = genome()
    rev = bool(k & 1)  # the anchor's strand
    off = 100 + int(rng.integers(0, 60))
    # forward intervals inside the unit: the anchor's stretch and, 330 bp downstream of its start, the mate's
    lo, hi = (off, off + 330) if not rev else (off + 330, off)
    anchor = ref[BASE_D + lo: BASE_D + lo + 150]
    mate = _mutate(rng, ref[BASE_D + hi: BASE_D + hi + 150], int(rng.integers(1, 4)))
    if rev:
        anchor = revcomp(anchor)
    else:
        mate = revcomp(mate)
    # 12 hits, best first: ten copies in random order, then two of the same copies again with the hit 500 bp further along its strand
    # (as a clipped or gapped alignment would lie).  From there the window cuts the mate's copy, Smith-Waterman finds a part of the
    # hit the proper anchor finds whole, and mem_sort_and_dedup has a redundant region to remove.
    order = rng.permutation(N_D)
    va = _vector([_region(_on_strand(BASE_D + STEP_D * int(order[j % 10]) + lo, 150, rev) + (500 if j >= 10 else 0), 150, 150 - j // 3, a)
                  for j in range(N_D)])
    vm = []
    if (k >> 1) & 1:
        for c in rng.choice(order[:10], N_D // 3, replace=False):
            vm.append(_region(_on_strand(BASE_D + STEP_D * int(c) + hi, 150, not rev), 141 - int(rng.integers(0, 4)), a))
    return _oriented(((anchor, va), (mate, _vector(vm))), bool((k >> 2) & 1))


def tandem(rng, a, k):
    _, _, ref = genome()
    rev = bool(k & 1)
    lm = 100 + int(rng.integers(0, 21))
    s = int(rng.integers(0, UNIT_T))
    # the mate lies over the anchor's own position: from anchor c the first full copy in the window is copy c's, which does not
    # reach the next anchor's insert-size range -- so every anchor needs its own invocation
    anchor = ref[BASE_T + s: BASE_T + s + 100]
    t = s + (0 if not rev else 100 - lm)
    mate = _mutate(rng, ref[BASE_T + UNIT_T + t: BASE_T + UNIT_T + t + lm], int(rng.integers(0, 3)))
    if rev:
        anchor = revcomp(anchor)
    else:
        mate = revcomp(mate)
    first = 1 if rev else 0  # (copy 0 has nothing upstream for a reverse-strand anchor's mate)
    # best first in the order in which no rescued mate covers a later anchor: a forward anchor's mate hit lies within the insert-size
    # range of the copies before it, a reverse anchor's of the copy after it
    copies = range(10) if not rev else range(9, -1, -1)
    va = _vector([_region(_on_strand(BASE_T + UNIT_T * (c + first) + s, 100, rev), 100 - j // 4, a) for j, c in enumerate(copies)])
    return _oriented(((anchor, va), (mate, _vector([]))), bool((k >> 1) & 1))


EDGE_RB = (5, L_PAC - 160, L_PAC - 20, L_PAC + 3, L_PAC + 400, 2 * L_PAC - 160, 2 * L_PAC - 100, 2 * L_PAC - LOW)


def edge(rng, a, k):
    _, _, ref = genome()
    rb, lm = EDGE_RB[k % len(EDGE_RB)], (80, 130, 150)[k // len(EDGE_RB) % 3]
    rev = rb >= L_PAC
    fb = rb if not rev else 2 * L_PAC - (rb + 100)  # the anchor's forward interval starts here (it may leave the strand: synthetic)
    mb = fb + 220 if not rev else fb - 220 - (lm - 100)  # a proper FR mate's forward interval, where the genome has one
    anchor = ref[fb: fb + 100] if 0 <= fb <= L_PAC - 100 else rng.integers(0, 4, 100).astype(np.uint8)
    mate = _mutate(rng, ref[mb: mb + lm], 2) if 0 <= mb <= L_PAC - lm else rng.integers(0, 4, lm).astype(np.uint8)
    if rev:
        anchor = revcomp(anchor)
    else:
        mate = revcomp(mate)
    return _oriented(((anchor, _vector([_region(rb, 100, 96, a)])), (mate, _vector([]))), bool((k >> 3) & 1))


def inactive(rng, a, k):
    """no rescue under the FR-only table: a proper FR pair, or a pair without any hit"""
    _, _, ref = genome()
    x = FREE0 + int(rng.integers(0, FREE1 - FREE0 - 600))
    r1, r2 = ref[x: x + 150].copy(), revcomp(ref[x + 330: x + 480])
    if k % 3 == 2:
        return [r1, r2], [_vector([]), _vector([])]
    return _oriented(((r1, _vector([_region(x, 150, 150, a)])), (r2, _vector([_region(_on_strand(x + 330, 150, True), 150, 147, a)]))), bool(k & 1))


def _flat(pairs):
    reads, regs = [], []
    for r, v in pairs:
        reads += r
        regs += v
    return reads, regs


@functools.lru_cache(maxsize=None)
def main_batch(scoring_name):
    """104 pairs: 40 dispersed, 40 tandem, 24 edge.  Returns (reads, regs), flat, 2 per pair."""
    a = int(scoring(scoring_name)["a"])
    rng = np.random.default_rng(77)
    pairs = [dispersed(rng, a, k) for k in range(40)] + [tandem(rng, a, k) for k in range(40)] + [edge(rng, a, k) for k in range(24)]
    return _flat([pairs[i] for i in rng.permutation(len(pairs))])


@functools.lru_cache(maxsize=None)
def mixed_batch(n_active, n_inactive, seed=5):
    """n_active pairs of the three families among n_inactive that need no rescue under the FR-only table (byte scoring)"""
    rng = np.random.default_rng(1000 * seed + n_active)
    makers = (dispersed, tandem, edge)
    pairs = [makers[k % 3](rng, 1, k + seed) for k in range(n_active)] + [inactive(rng, 1, k) for k in range(n_inactive)]
    return _flat([pairs[i] for i in rng.permutation(len(pairs))])


def bmh_dedup_callback(level, counter=None):
    """bmh_sort_and_dedup(n, a, level) with the bmh_dedup_fn shape; counter (a list of one int): regions removed so far."""
    import ctypes as C

    from __graft_entry__ import load_package
    lib = load_package().lib()
    lib.bmh_sort_and_dedup.restype = C.c_int
    lib.bmh_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]

    def cb(_user, n, a):
        m = lib.bmh_sort_and_dedup(n, a, level)
        if counter is not None:
            counter[0] += n - m
        return m
    return kswlib.DEDUP_FN(cb)


@functools.lru_cache(maxsize=None)
def oracle(batch, scoring_name, table, opt_name):
    """The oracle's mate rescue (orc_matesw_pair per pair, mem_sort_and_dedup = bmh_sort_and_dedup at LEVEL) over a batch, computed once:
    batch is "main" or (n_active, n_inactive).  Returns (regs after rescue, n per pair, regions de-duplication removed)."""
    l_pac, pac, _ = genome()
    reads, regs = main_batch(scoring_name) if batch == "main" else mixed_batch(*batch)
    removed = [0]
    cb = bmh_dedup_callback(LEVEL, removed)
    want, ns = kswlib.orc_matesw_pairs(scoring(scoring_name), opt(opt_name), l_pac, pac, pes(table), reads, regs, cb)
    return want, ns, removed[0]
