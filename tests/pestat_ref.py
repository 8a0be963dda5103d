"""mem_pestat's pair walk restated plainly in Python (reference bwa-0.7.8/bwamem_pair.c:23-62: mem_infer_dir, cal_sub and the tests
of the loop), the hand-made vectors that reach every exit and edge of that rule, and helpers the CPU and GPU tests share.

The word of a pair: 0 = no candidate, else orientation << 30 | insert size.  word() also names what the pair met on its way (a set of
tags), so that a test can count from this restatement alone that every class occurs."""
import numpy as np

import kswlib

MIN_RATIO = 0.8  # bwamem_pair.c:14


def infer_dir(l_pac, b1, b2):
    """bwamem_pair.c:23-30 -> (orientation, distance)"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else (l_pac << 1) - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), (p2 - b1 if p2 > b1 else b1 - p2)


def cal_sub(o, a, tags, who):
    """bwamem_pair.c:32-44; the comparison is C's: int against the single-precision product of an int and mask_level"""
    mask = np.float32(o["mask_level"])
    overlapped = False
    for j in range(1, len(a)):
        b_max, e_min = max(int(a[j]["qb"]), int(a[0]["qb"])), min(int(a[j]["qe"]), int(a[0]["qe"]))
        if e_min > b_max:
            overlapped = True
            min_l = min(int(a[j]["qe"]) - int(a[j]["qb"]), int(a[0]["qe"]) - int(a[0]["qb"]))
            thr = np.float32(min_l) * mask
            if np.float32(e_min - b_max) >= thr:
                if np.float32(e_min - b_max) == thr:
                    tags.add("ovl_exact")
                if j == len(a) - 1 and len(a) >= 40:
                    tags.add("hit_last_of_40")
                return int(a[j]["score"])
            if np.float32(e_min - b_max + 1) >= thr:
                tags.add("ovl_one_less")
    if len(a) > 1 and not overlapped:
        tags.add("no_overlap")
    return int(o["min_seed_len"]) * int(o["a"])


def word(o, l_pac, a0, a1):
    """bwamem_pair.c:56-62 for one pair -> (word, tags)"""
    tags = set()
    if len(a0) == 0 or len(a1) == 0:
        tags.add("empty0" if len(a0) == 0 else "empty1")
        return 0, tags
    for k, a in enumerate((a0, a1)):
        sub, lim = cal_sub(o, a, tags, k), MIN_RATIO * float(int(a[0]["score"]))
        if int(a[0]["score"]) % 5 == 0 and sub == int(a[0]["score"]) * 4 // 5:
            tags.add(f"sub{k}_at")
        if int(a[0]["score"]) % 5 == 0 and sub == int(a[0]["score"]) * 4 // 5 + 1:
            tags.add(f"sub{k}_above")
        if sub > lim:
            tags.add(f"sub{k}_reject")
            return 0, tags
    b1, b2 = int(a0[0]["rb"]), int(a1[0]["rb"])
    d, dist = infer_dir(int(l_pac), b1, b2)
    tags.add(f"r0_{'rev' if b1 >= l_pac else 'fwd'}"), tags.add(f"r1_{'rev' if b2 >= l_pac else 'fwd'}")
    if dist == 0:
        tags.add("is0")
    if dist == int(o["max_ins"]):
        tags.add("is_max")
    if dist == int(o["max_ins"]) + 1:
        tags.add("is_max1")
    if dist and dist <= int(o["max_ins"]):
        tags.add(f"dir{d}")
        return d << 30 | dist, tags
    return 0, tags


def words(o, l_pac, vecs):
    """-> (uint32 words of the n // 2 pairs, the union count of tags)"""
    out, seen = np.zeros(len(vecs) // 2, dtype=np.uint32), {}
    for p in range(len(vecs) // 2):
        w, tags = word(o, l_pac, vecs[2 * p], vecs[2 * p + 1])
        out[p] = w
        for t in tags:
            seen[t] = seen.get(t, 0) + 1
    return out, seen


def reg(rb, qb=0, qe=100, score=60, truesc=None):
    a = np.zeros(1, dtype=kswlib.ALNREG)
    a["rb"], a["re"], a["qb"], a["qe"], a["score"] = rb, rb + (qe - qb), qb, qe, score
    a["truesc"] = score if truesc is None else truesc
    return a


def vec(*regs):
    return np.concatenate(regs) if regs else np.zeros(0, dtype=kswlib.ALNREG)


def mate_rb(l_pac, b1, d, dist):
    """the head position of mate 2 that gives orientation d at distance dist from mate 1's head at b1 (dist 0: same place)"""
    p2 = b1 + dist if d in (0, 1) else b1 - dist
    return p2 if d in (0, 3) else (l_pac << 1) - 1 - p2


def pair_of(l_pac, d, dist, b1=None, score=60):
    """two one-region vectors whose word is d << 30 | dist"""
    b1 = l_pac // 2 if b1 is None else b1
    return [reg(b1, score=score), reg(mate_rb(l_pac, b1, d, dist), score=score)]


ALL_TAGS = ("empty0", "empty1", "sub0_at", "sub0_above", "sub1_at", "sub1_above", "sub0_reject", "sub1_reject", "ovl_exact", "ovl_one_less",
            "no_overlap", "is0", "is_max", "is_max1", "dir0", "dir1", "dir2", "dir3", "r0_fwd", "r0_rev", "r1_fwd", "r1_rev", "hit_last_of_40")


def handmade(o, l_pac):
    """Vectors (2 per pair) for every exit and edge of the rule; which is which is told by word()'s tags, not by position."""
    mi, msa = int(o["max_ins"]), int(o["min_seed_len"]) * int(o["a"])
    mask = float(np.float32(o["mask_level"]))
    ovl = int(round(100 * mask))  # two 100-base regions: the overlap at which e_min - b_max == min_l * mask_level
    assert np.float32(ovl) == np.float32(100) * np.float32(o["mask_level"]), "choose a mask_level with 100 * mask_level whole"
    b = l_pac // 2
    good = reg(b + 300)
    v = []
    v += [vec(), good, good, vec(), vec(), vec()]  # an empty mate, either side, both
    for side in (0, 1):  # sub exactly at, and one above, 0.8 * score with score a multiple of 5
        for score in (50, 55, 100):
            for extra in (0, 1):
                sub = score * 4 // 5 + extra
                tested = vec(reg(b, score=score), reg(b + 5000, score=sub))  # fully overlapping second region
                v += [tested, good] if side == 0 else [reg(b - 300), tested]
    # an overlap of exactly min_l * mask_level (cal_sub takes that region's score, here too high), and one base less (it does not)
    for shift in (100 - ovl, 100 - ovl + 1):
        other = reg(b + 9000, qb=shift, qe=shift + 100, score=59)
        v += [vec(reg(b, score=60), other), good, reg(b - 200), vec(reg(b, score=60), other)]
    # ... with the shorter region deciding min_l
    v += [vec(reg(b, score=60), reg(b + 9000, qb=60, qe=100, score=59)), good]
    # no overlapping region at all: sub = min_seed_len * a, against scores around it
    for score in (msa, msa + msa // 4, msa + msa // 4 + 1, 2 * msa):
        v += [vec(reg(b, qb=0, qe=50, score=score), reg(b + 700, qb=50, qe=100, score=score), reg(b + 900, qb=70, qe=100, score=score)), good]
    # insert size 0, max_ins, max_ins + 1, in all four orientations, mate 1 on either side of l_pac
    for b1 in (b, l_pac + b, l_pac - 1, l_pac, 0 + mi + 2, 2 * l_pac - mi - 3):
        for d in range(4):
            for dist in (0, 1, mi, mi + 1, 137):
                rb2 = mate_rb(l_pac, b1, d, dist)
                if 0 <= rb2 < 2 * l_pac:
                    v += [reg(b1), reg(rb2)]
    # cal_sub's hit on the last region of a 40-region vector: 38 regions that do not overlap the head, then one that does
    far = [reg(b + 100 * k, qb=100, qe=150, score=10) for k in range(38)]
    for last_score in (59, 48, 49):
        v += [vec(reg(b, score=60), *far, reg(b + 8000, score=last_score)), good, reg(b - 250), vec(reg(b, score=60), *far, reg(b + 8000, score=last_score))]
    v += [vec(reg(b, score=60), reg(b + 5, score=30)), vec(reg(b + 210, score=60), reg(b + 7, score=30))]  # 2 regions each, a candidate
    return v


def drop_exact(vecs, lens, match):
    """mem_test_and_remove_exact with MEM_F_NO_EXACT set (bwamem.c:438-443) -> (vectors, regions removed)"""
    out, gone = [], 0
    for a, l in zip(vecs, lens):
        if len(a) and int(a[0]["truesc"]) == int(l) * int(match):
            a, gone = a[1:], gone + 1
        out.append(a.copy())
    return out, gone


def digest(w):
    """what tests/pestat_core_main.c prints of its words: sum of (word + golden) * (2 i + 1) modulo 2^64"""
    w = np.asarray(w, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((w + np.uint64(0x9E3779B97F4A7C15)) * (np.arange(len(w), dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))


def random_vectors(rng, n_pairs, l_pac, max_ins, exact_share=0.0, L=100, match=1):
    """2 * n_pairs small vectors (0-3 regions) around candidate-making placements, cheap to build in bulk; returns (vectors, lengths)"""
    n = 2 * n_pairs
    cnt = rng.choice([0, 1, 1, 1, 2, 2, 3], size=n)
    off = np.concatenate([[0], np.cumsum(cnt)])
    flat = np.zeros(int(off[-1]), dtype=kswlib.ALNREG)
    m = len(flat)
    flat["qb"] = rng.integers(0, 60, m)
    flat["qe"] = flat["qb"] + rng.integers(20, L - 59, m)
    flat["score"] = rng.integers(15, 101, m)
    flat["truesc"] = np.where(rng.random(m) < exact_share, L * match, flat["score"])
    flat["rb"] = rng.integers(0, 2 * l_pac, m)
    head = off[:-1][cnt > 0]
    flat["score"][head] = rng.choice([50, 55, 60, 75, 100], len(head))
    # mate 2's head near mate 1's, in a random orientation
    pp = np.nonzero((cnt[0::2] > 0) & (cnt[1::2] > 0))[0]
    b1 = rng.integers(2 * max_ins, l_pac - 2 * max_ins, len(pp)) + l_pac * (rng.random(len(pp)) < 0.5)
    d, dist = rng.integers(0, 4, len(pp)), rng.integers(0, max_ins + max_ins // 8, len(pp))
    p2 = np.where(d <= 1, b1 + dist, b1 - dist)  # mate_rb, for arrays
    flat["rb"][off[2 * pp]] = b1
    flat["rb"][off[2 * pp + 1]] = np.where((d == 0) | (d == 3), p2, 2 * l_pac - 1 - p2)
    flat["re"] = flat["rb"] + (flat["qe"] - flat["qb"])
    return [flat[off[i]:off[i + 1]] for i in range(n)], np.full(n, L, dtype=np.int32)
