"""Seeded generator of pass B's inputs on a small multi-contig reference: reads cut from the concatenation (mutated with
kswgen.mutate, both strands), region vectors with chosen qb, qe, rb, re, truesc and w -- pass B reads nothing else of a region, so
truesc steers the bands -- want lists of zero to six regions per read, and constructed regions that hang over the end of their
reference sequence, bridge the strands or lose everything to bwa_fix_xref2."""
import numpy as np

import kswgen
import kswlib

CONTIG_LENS = (3000, 1001, 507)
CONTIGS = [(sum(CONTIG_LENS[:i]), n) for i, n in enumerate(CONTIG_LENS)]
L_PAC = sum(CONTIG_LENS)
BOUNDS = [CONTIGS[1][0], CONTIGS[2][0]]  # where one sequence ends and the next begins


def pack(bases):
    pad = np.concatenate([bases, np.zeros(4, np.uint8)])
    q4 = pad[: (len(pad) // 4) * 4].reshape(-1, 4)
    return (q4[:, 0] << 6 | q4[:, 1] << 4 | q4[:, 2] << 2 | q4[:, 3]).astype(np.uint8)


def reference(seed=5):
    whole = kswgen.rand_seq(np.random.default_rng(seed), L_PAC)
    return whole, pack(whole)


def revcomp(s):
    return (3 - np.asarray(s, dtype=np.uint8)[::-1]).astype(np.uint8)


def region(qb, qe, rb, re, truesc, w, score=0):
    a = np.zeros((), dtype=kswlib.ALNREG)
    a["qb"], a["qe"], a["rb"], a["re"], a["truesc"], a["w"], a["score"], a["secondary"] = qb, qe, rb, re, truesc, w, score, -1
    return a


def long_fixes(whole, b, score=0):
    """Two regions over the boundary b between two sequences of `whole` whose one-try alignment outgrows its 24-word slot, so that the
    host redoes them, fix included: 14 separated indels on the way to b, then 60 bases past it, forwards and reverse-complemented
    -> [(read, region)]"""
    parts, at = [], b - 300
    for j in range(14):
        parts.append(whole[at:at + 20])
        at += 20
        if j % 2:
            parts.append(np.array([(int(whole[at]) + 2) & 3, (int(whole[at]) + 1) & 3], dtype=np.uint8))
        else:
            at += 2
    parts.append(whole[at:b + 60])
    rd, l2 = np.concatenate(parts), 2 * len(whole)
    return [(rd, region(0, len(rd), b - 300, b + 60, len(rd) - 50, 100, score)),
            (revcomp(rd), region(0, len(rd), l2 - b - 60, l2 - b + 300, len(rd) - 50, 100, score))]


def on_strand(rb, re, rev):
    return (2 * L_PAC - re, 2 * L_PAC - rb) if rev else (rb, re)


KINDS = ("exact", "two", "three", "nogap", "shared")


def edit(rng, src, n_sub, indels=()):
    """src with n_sub substitutions and the given indels, (position, length): length > 0 inserts random bases, < 0 deletes"""
    seg = src.copy()
    for i in rng.choice(len(seg), size=min(n_sub, len(seg)), replace=False):
        seg[i] = (int(seg[i]) + int(rng.integers(1, 4))) & 3
    for pos, ln in sorted(indels, reverse=True):
        seg = np.concatenate([seg[:pos], kswgen.rand_seq(rng, ln), seg[pos:]]) if ln > 0 else np.concatenate([seg[:pos], seg[pos - ln:]])
    return seg.astype(np.uint8)


def segment(rng, whole, kind, ln):
    """A read segment cut from inside one sequence and its region: (bases, rb, re, truesc, w).  Few enough events for 24 CIGAR words
    and 96 MD bytes, and never an alignment forced through a band too narrow for its indels."""
    off, n = CONTIGS[int(rng.integers(0, len(CONTIGS)))]
    ln = max(min(ln, n - 20), 20)
    if kind == "three":
        ln = max(ln, 130)
    pos = off + int(rng.integers(5, n - ln - 5))
    src = whole[pos:pos + ln]
    if kind == "nogap":  # ql == tl and the score within a gap's cost of perfect: no alignment at all (bwa.c:108-114)
        return edit(rng, src, int(rng.integers(0, 2))), pos, pos + ln, ln - int(rng.integers(0, 6)), 100
    if kind == "exact":  # at or under the true score, at most one indel: one try
        one = [(int(rng.integers(5, ln - 5)), int(rng.choice([-2, -1, 1, 2])))] if rng.random() < 0.5 else []
        seg = edit(rng, src, int(rng.integers(1, 4)), one)
        return seg, pos, pos + ln, min(len(seg), ln) - 14 - int(rng.integers(0, 30)), 100
    if kind == "two":  # the estimate says perfect, an indel and a substitution say otherwise: a second try with the same score
        seg = edit(rng, src, 1, [(int(rng.integers(5, ln - 5)), int(rng.choice([-3, -1, 2])))])
        return seg, pos, pos + ln, min(len(seg), ln), 100
    if kind == "three":  # bands 3, 6, 12 (the inferred band capped by the region's 3): a pair of 5-base indels fits the second, of 12 the third
        seg = edit(rng, src, 0, [(15, -5), (35, 5), (60, -12), (ln - 25, 12)])
        return seg, pos, pos + ln, ln - 120, 3
    # "shared": substitutions only; the region's band of 1 or 2 caps the inferred one: bands 3, 3, 4 or 3, 3, 8 -- tries share a task
    return edit(rng, src, int(rng.integers(0, 4))), pos, pos + ln, ln - 120, int(rng.choice([1, 2]))


def random_slice(rng, whole, n_reads, first_last_want=True, empty_every=5):
    """-> (reads, vectors, want): reads with zero to six regions; wants of zero to six per read, not in index order"""
    reads, vectors, want = [], [], []
    for i in range(n_reads):
        edge = first_last_want and i in (0, n_reads - 1)
        n_seg = int(rng.choice([1, 1, 1, 2, 3, 6])) if edge or i % empty_every else 0
        segs, regs, q = [], [], 0
        for _ in range(n_seg):
            rev = bool(rng.integers(0, 2))
            seg, rb, re, truesc, w = segment(rng, whole, KINDS[int(rng.integers(0, len(KINDS)))], int(rng.integers(30, 160)))
            rb, re = on_strand(rb, re, rev)
            segs.append(revcomp(seg) if rev else seg)
            regs.append(region(q, q + len(seg), rb, re, truesc, w))
            q += len(seg)
        reads.append(np.concatenate(segs) if segs else kswgen.rand_seq(rng, 50))
        vectors.append(np.array(regs, dtype=kswlib.ALNREG).reshape(-1))
        ks = list(rng.permutation(n_seg))
        if not edge and n_seg and rng.random() < 0.2:
            ks = ks[:int(rng.integers(0, n_seg))]  # some regions, or none, of a read that has them
        want.append([int(k) for k in ks])
    return reads, vectors, want


def slice_of(rng, whole, n_wanted):
    """a slice with exactly n_wanted wanted regions"""
    reads, vectors, want = random_slice(rng, whole, max(n_wanted, 2))
    total = 0
    for i, ks in enumerate(want):
        if total + len(ks) > n_wanted:
            want[i] = ks[:n_wanted - total]
        total += len(want[i])
    last = max(i for i, ks in enumerate(want) if ks) + 1
    return reads[:last], vectors[:last], want[:last]


def overhangs(whole):
    """Constructed regions over the ends of reference sequences -> list of (name, read, region, expect) with expect one of
    "Mb", "Me" (the cut falls in a match run at the left / right end), "Db", "De" (inside a deletion), "none" (no fix needed), "-2"
    (nothing is left: the call fails), "bridge" (across the strands: the call fails).  Error-free reads, forwards and
    reverse-complemented, the midpoint on either side of the boundary."""
    out = []

    def add(name, rd, rb, re, expect, rev):
        rb2, re2 = on_strand(rb, re, rev)
        if rev and expect in ("Mb", "Me", "Db", "De"):  # on the other strand left and right swap
            expect = expect[0] + ("e" if expect[1] == "b" else "b")
        out.append((f"{name}{'-' if rev else '+'}", revcomp(rd) if rev else rd, region(0, len(rd), rb2, re2, len(rd), 100, len(rd)), expect))
    for b in BOUNDS:
        for rev in (False, True):
            for left, right in ((70, 40), (40, 70), (25, 110), (110, 25)):  # plain overhangs: the shorter side is cut off
                add(f"plain{b}:{left}/{right}", whole[b - left:b + right], b - left, b + right, "Mb" if right > left else "Me", rev)
            # a deletion that spans the boundary: the cut falls inside the D operation (bwa.c:210-216)
            add(f"delL{b}", np.concatenate([whole[b - 58:b - 2], whole[b + 3:b + 95]]), b - 58, b + 95, "Db", rev)
            add(f"delR{b}", np.concatenate([whole[b - 95:b - 3], whole[b + 2:b + 58]]), b - 95, b + 58, "De", rev)
            add(f"delL'{b}", np.concatenate([whole[b - 40:b - 1], whole[b + 6:b + 120]]), b - 40, b + 120, "Db", rev)
            add(f"delR'{b}", np.concatenate([whole[b - 120:b - 6], whole[b + 1:b + 40]]), b - 120, b + 40, "De", rev)
            # an insertion next to the boundary
            ins = ((whole[b - 1:b + 2] + 1) & 3).astype(np.uint8)
            add(f"insL{b}", np.concatenate([whole[b - 40:b - 1], ins, whole[b - 1:b + 90]]), b - 40, b + 90, "Mb", rev)
            add(f"insR{b}", np.concatenate([whole[b - 90:b + 1], ins, whole[b + 1:b + 40]]), b - 90, b + 40, "Me", rev)
            # up to the boundary and no further: nothing to fix
            add(f"touchL{b}", whole[b - 80:b], b - 80, b, "none", rev)
            add(f"touchR{b}", whole[b:b + 80], b, b + 80, "none", rev)
    return out


def lost_regions(whole):
    """Regions of which bwa_fix_xref2 leaves nothing (qb == qe, bwa.c:221) -> list of (name, read, region): 40 bases that end (begin) at
    a boundary with a window 60 bases longer on the far side, so that the midpoint lies in the next (previous) sequence and the whole
    query is aligned outside it, behind (in front of) a 60-base deletion.  Both boundaries, forward strand."""
    out = []
    for b in BOUNDS:
        for rev in (False,):  # (a hit on the reverse strand is aligned backwards and its CIGAR walked forwards: something is left of it)
            for name, rd, rb, re in (("lostL", whole[b - 40:b], b - 40, b + 60), ("lostR", whole[b:b + 40], b - 60, b + 40)):
                rb2, re2 = on_strand(rb, re, rev)
                out.append((f"{name}{b}{'-' if rev else '+'}", revcomp(rd) if rev else rd.copy(), region(0, 40, rb2, re2, 40, 100, 40)))
    return out


def lost_region(whole):
    return lost_regions(whole)[0][1:]


def bridging_region(whole):
    return whole[L_PAC - 30:].copy(), region(0, 30, L_PAC - 30, L_PAC + 30, 30, 100, 30)
