"""Seeded slices for the redo path of the fused phase 2 session (bmh_phase2_text_device): regions whose alignments outgrow the device's
slots -- an MD past 128 bytes or a CIGAR past 24 words -- in the numbers and places where that path branches.
 * growth_slice: a few reads of tens of thousands of bases with a substitution every second or third base, so that the redone regions'
   MD strings together pass the megabytes pass B's block has to spare and the overflow area behind it has to grow; with the
   arithmetic of that block (wanted_block, Block::take, ensure and ensure_keep of csrc/api.hip restated) and the MD length a gapless
   alignment gives, so that a test can say before any GPU runs whether the slice reaches the branch.
 * counted_slice: exactly m redone regions of 250 bases at irregular places among ordinary reads, on wantgen's reference.
 * paired_slice: pairs of which one mate, the other, both or the only mapped one is redone.
Nothing here needs a GPU."""
import numpy as np

import kswlib
import phase2gen as pg
import wantgen as wg

MIB = 1 << 20
MD_SLOT, CIGAR_SLOT = 128, 24  # what a record's slots hold (BMH_RP_MD_SLOT bytes, BMH_RP_SMALL_CAP words)
RECORD, PLACE = 72, 8          # per redone region in the overflow area: its bmh_wanted_res_t and its place in want order
# pass B's block per region of the slice, section by section (wanted_block): WantRec, 4 keys, 4 sums, 2 requests, round 0's result, CIGAR
# slot and MD slot, the main round's result, the record, and the main round's CIGAR and MD slots
PER_REGION = (80, 4, 4, 4, 4, 8, 8, 8, 8, 48, 48, 24, 96, 4, 24, 72, 96, 128)
STATUS = 2 * 64


def ceil_mib(x):
    return (int(x) + MIB - 1) // MIB * MIB


def take(x):
    """Block::take: every section of a device block is rounded up to 64 bytes"""
    return (int(x) + 63) & ~63


def lb_end(n, regions):
    """wanted_block's end for a slice of n reads and `regions` regions: first[], the per-region sections with the two status records
    between them.  (Where the status stands does not change the sum.)"""
    return take(8 * (n + 1)) + sum(take(regions * s) for s in PER_REGION) + take(STATUS)


def lb_max(n, regions):
    """An upper bound on lb_end that needs no knowledge of the sections: 8 bytes per read and 1024 per region plus 4096.  The sections
    hold 8 * (n + 1) + 128 + 668 * regions bytes (sum(PER_REGION) == 668), and each of the twenty is rounded up by at most 63 bytes:
    8 + 128 + 20 * 63 = 1396 < 4096, and 668 < 1024."""
    return 8 * n + 1024 * regions + 4096


def first_cap(lb):
    """what ensure() allocates for a block of lb bytes on a context that has none: a quarter more, rounded up to a MiB"""
    return ceil_mib(lb + lb // 4)


def grown_cap(cap, o_end):
    """ensure_keep for o_end > cap: ensure() on a fresh buffer for max(o_end, 2 * cap) -> (the new capacity, whether o_end decided it)"""
    want = max(o_end, 2 * cap)
    return ceil_mib(want + want // 4), o_end > 2 * cap


def overflow_bytes(md_len, n_cigar):
    """the overflow area of the regions past their slots, without its sections' rounding: a record and a place each, the CIGAR words, the
    MD bytes -> (bytes, regions)"""
    md_len, n_cigar = np.asarray(md_len, dtype=np.int64), np.asarray(n_cigar, dtype=np.int64)
    past = (md_len > MD_SLOT) | (n_cigar > CIGAR_SLOT)
    m = int(past.sum())
    return m * (RECORD + PLACE) + 4 * int(n_cigar[past].sum()) + int(md_len[past].sum()), m


def md_len_gapless(length, subs):
    """the length of the MD string of `length` bases aligned without a gap with mismatches at the sorted positions `subs`: per mismatch
    the digits of the run of matches before it and the reference base, then the digits of the last run (bwa.c:134-164)"""
    subs = np.asarray(subs, dtype=np.int64)
    runs = np.diff(np.concatenate([[-1], subs, [length]])) - 1
    digits = np.ones(len(runs), dtype=np.int64)
    for p in (10, 100, 1000, 10000, 100000):
        digits += runs >= p
    return int(digits.sum()) + len(subs)


# ---------------------------------------------------------------- a reference that holds long windows and phase2gen's slices

def long_reference(l_pac, seed):
    """l_pac bases in two sequences of half each.  The first begins with wantgen's reference and its reverse complement, so that a region
    phase2gen placed at a doubled coordinate of that reference (both strands: wg.on_strand) lies on the same bases here, on the forward
    strand of the first sequence: an ordinary slice of phase2gen.make is an ordinary slice on this reference too.
    -> (bases, contigs)"""
    small, _ = wg.reference()
    assert l_pac // 2 >= 2 * wg.L_PAC + 1000
    rest = np.random.default_rng(seed).integers(0, 4, size=l_pac - 2 * wg.L_PAC, dtype=np.uint8)
    return np.concatenate([small, wg.revcomp(small), rest]), [(0, l_pac // 2), (l_pac // 2, l_pac - l_pac // 2)]


LONG, ALIGNED = 60000, 12000  # bases of a long read without and with a banded alignment; windows of the same length, under 65 535


def _strand(l_pac, pos, tl, rev):
    return (2 * l_pac - pos - tl, 2 * l_pac - pos) if rev else (pos, pos + tl)


def _substituted(whole, pos, length, step):
    rd = whole[pos:pos + length].copy()
    subs = np.arange(1, length, step)
    rd[subs] = (rd[subs] + 1 + (subs // step) % 3) & 3
    return rd, subs


def growth_slice(whole, l_pac, n_direct, n_aligned, seed):
    """n_direct reads of LONG bases with every second base substituted, whose region says the perfect score, so that mem_reg2aln takes
    the alignment without a gap and without a DP (bwa.c:108-114): an MD of one byte per base at no cost to the host.  n_aligned reads
    of ALIGNED bases with every third base substituted and a true score 12 under perfect: bands 8, 16 and 32 through ksw_global2, the
    length test_wanted_device_gpu.py runs the long-task kernels at.  Both strands, both sequences; after every second long read an
    ordinary read of 150 bases, so that patched and unpatched records alternate in want order.
    -> (reads, vectors, info): info["md_len"] the gapless MD length per long read, info["window"] every region's window length"""
    rng = np.random.default_rng(seed)
    half = l_pac // 2
    reads, vectors, md_len, window = [], [], [], []
    n_long = n_direct + n_aligned
    every = max(n_long // max(n_aligned, 1), 1)
    left = n_aligned
    for i in range(n_long):
        aligned = left > 0 and i % every == every // 2
        left -= aligned
        length, step = (ALIGNED, 3) if aligned else (LONG, 2)
        base = half * (i % 2)
        lo = 2 * wg.L_PAC if base == 0 else 50
        pos = base + lo + int(rng.integers(0, half - length - lo - 50))
        rd, subs = _substituted(whole, pos, length, step)
        rev = bool((i // 2) & 1)
        rb, re = _strand(l_pac, pos, length, rev)
        reg = wg.region(0, length, rb, re, length - 12 if aligned else length, 100, length - 40)
        reg["seedcov"] = 60
        reads.append(wg.revcomp(rd) if rev else rd), vectors.append(np.array([reg], dtype=kswlib.ALNREG))
        md_len.append(md_len_gapless(length, subs)), window.append(length)
        if i % 2:
            pos = half * int(rng.integers(0, 2)) + 2 * wg.L_PAC + int(rng.integers(0, half - 2 * wg.L_PAC - 200))
            rd = wg.edit(rng, whole[pos:pos + 150], 3)
            rev = bool(rng.integers(0, 2))
            rb, re = _strand(l_pac, pos, 150, rev)
            reg = wg.region(0, 150, rb, re, 110, 100, 110)
            reg["seedcov"] = 60
            reads.append(wg.revcomp(rd) if rev else rd), vectors.append(np.array([reg], dtype=kswlib.ALNREG))
            window.append(150)
    assert left == 0
    return reads, vectors, dict(md_len=md_len, window=window, n_long=n_long)


def predicted_overflow(info):
    """the overflow area the slice's long reads need if every one is aligned without a gap: one CIGAR word each"""
    return overflow_bytes(info["md_len"], [1] * len(info["md_len"]))[0]


REFERENCE = dict(l_pac=150000, seed=81)
FIRST = dict(n_direct=27, n_aligned=5, seed=181)    # the slice that grows a fresh context's block
SECOND = dict(n_direct=125, n_aligned=5, seed=182)  # past twice the capacity the first leaves behind


def growth_reference():
    return long_reference(**REFERENCE)


def growth(whole, spec):
    return growth_slice(whole, len(whole), **spec)


# ---------------------------------------------------------------- redone regions of 250 bases, on wantgen's reference

def _md_read(whole, pos):
    """a substitution every third base of 250: an MD of about 170 bytes"""
    rd = whole[pos:pos + 250].copy()
    rd[::3] = (rd[::3] + 1) & 3
    return rd, 250


def _cigar_read(whole, pos):
    """alternately a base deleted and a base inserted, 14 times, 30 bases apart: a CIGAR of 29 words"""
    parts, at = [], pos
    for j in range(14):
        parts.append(whole[at:at + 30])
        at += 30
        if j % 2:
            parts.append(np.array([(int(whole[at]) + 2) & 3, (int(whole[at]) + 1) & 3], dtype=np.uint8))
        else:
            at += 2
    parts.append(whole[at:at + 30])
    return np.concatenate(parts), at + 30 - pos


CIGAR_TL = 14 * 30 + 7 * 2 + 30  # the window of _cigar_read


def redone_read(whole, pos, rev, cigar):
    """-> (read, region): one region over the whole read whose alignment outgrows its MD slot, or (cigar) its CIGAR slot"""
    rd, tl = (_cigar_read if cigar else _md_read)(whole, pos)
    rb, re = wg.on_strand(pos, pos + tl, rev)
    reg = wg.region(0, len(rd), rb, re, len(rd) - 40, 100, len(rd) - 40)
    reg["seedcov"] = 60
    return (wg.revcomp(rd) if rev else rd), reg


def counted_slice(whole, m, seed):
    """m redone regions -- about one in four by its CIGAR, both strands, one in three the second region of its vector behind a
    lower-scoring one that the sort moves back -- dropped at random places into a slice of phase2gen's ordinary reads: runs of
    redone regions of every length, single ones, ordinary reads between.  -> (reads, vectors)"""
    rng = np.random.default_rng([seed, m])
    off, n = wg.CONTIGS[0]
    reads, vectors = pg.se_slice(rng, whole, m // 2 + 40)
    reads, vectors = list(reads), list(vectors)
    at = np.sort(rng.integers(0, len(reads) + 1, size=m))
    for t in range(m - 1, -1, -1):  # from the back, so that the places stay what they were
        cigar = bool(rng.random() < 0.25)
        pos = off + int(rng.integers(5, n - (CIGAR_TL if cigar else 250) - 5))
        rd, reg = redone_read(whole, pos, bool(rng.integers(0, 2)), cigar)
        if t % 3 == 1:
            opos = wg.CONTIGS[1][0] + int(rng.integers(5, wg.CONTIGS[1][1] - 130))
            other = wg.region(0, 120, opos, opos + 120, 110, 100, 100)
            other["seedcov"] = 60
            reg["qb"], reg["qe"] = 120, 120 + len(rd)
            rd, v = np.concatenate([whole[opos:opos + 120], rd]), np.array([other, reg], dtype=kswlib.ALNREG)
        else:
            v = np.array([reg], dtype=kswlib.ALNREG)
        reads.insert(int(at[t]), rd), vectors.insert(int(at[t]), v)
    return reads, vectors


PAIR_KINDS = ("redone+ordinary", "ordinary+redone", "redone+redone", "redone+none", "none+redone", "ordinary+ordinary", "cigar+ordinary",
              "ordinary+cigar")


def paired_slice(whole, n_pairs, seed):
    """FR pairs inside wantgen's longest sequence, the forward mate in front: per pair the kinds of PAIR_KINDS in turn -- a redone mate
    (by its MD; "cigar": by its CIGAR) beside an ordinary one, two redone mates, a redone mate beside one without any region -- and
    about a third of the pairs with the reverse read first.  -> (reads, vectors, kinds), 2 * n_pairs reads"""
    rng = np.random.default_rng([seed, n_pairs])
    off, n = wg.CONTIGS[0]
    reads, vectors, kinds = [], [], []
    for p in range(n_pairs):
        kind = PAIR_KINDS[p % len(PAIR_KINDS)]
        ka, kb = kind.split("+")
        tl = [CIGAR_TL if k == "cigar" else 250 if k == "redone" else int(rng.integers(60, 110)) for k in (ka, kb)]
        ins = tl[0] + tl[1] + int(rng.integers(0, 120))
        pos0 = off + int(rng.integers(5, n - ins - 5))
        ends = []
        for k, pos, ln, rev in ((ka, pos0, tl[0], False), (kb, pos0 + ins - tl[1], tl[1], True)):
            if k == "none":
                ends.append((rng.integers(0, 4, size=60, dtype=np.uint8), np.zeros(0, dtype=kswlib.ALNREG)))
            elif k == "ordinary":
                b, reg = pg._mate(rng, whole, pos, ln, rev)
                ends.append((b, pg.dress(rng, [reg], high=True)))
            else:
                b, reg = redone_read(whole, pos, rev, k == "cigar")
                ends.append((b, np.array([reg], dtype=kswlib.ALNREG)))
        if rng.random() < 0.3:
            ends.reverse()
        for b, v in ends:
            reads.append(b), vectors.append(v)
        kinds.append(kind)
    return reads, vectors, kinds
