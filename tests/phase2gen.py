"""Seeded slices for the fused phase 2 call (bmh_phase2_device): reads that align where their regions say, as wantgen makes them, with
what pass A decides on -- scores on both sides of T with ties, lower-scoring copies of a region over the same query interval (they
become secondaries), the order within a vector shuffled so that the sort moves regions -- and, paired-end, mates at FR distances
inside one sequence under an insert-size model with FR open, beside pairs no proper pair can be formed from.  bmh_decide_batch (the
host, no GPU) trims a slice to an exact number of wanted regions and counts the shapes the tests assert."""
import numpy as np

import decidegen as dg
import kswgen
import kswlib
import wantgen as wg
from __graft_entry__ import load_package

T = 30  # mem_opt_init's (decidegen.sam_opt)
PE, ALL = dg.PE, dg.ALL


def opt(w=100, flag=0):
    return dg.sam_opt(w=w, flag=flag)


def pes_fr():
    """FR open with inserts of 300 +- 80 inside 1..900; the other three orientations failed"""
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    pes["failed"] = 1
    pes[1]["failed"], pes[1]["low"], pes[1]["high"], pes[1]["avg"], pes[1]["std"] = 0, 1, 900, 300.0, 80.0
    return pes


N_TERM = 900  # entries of pes_fr()'s pair table


def _score(rng, ql, high=False):
    pool = [T + 15, 60, ql, ql] if high else [T - 9, T - 1, T - 1, T, T, T + 1, T + 15, 60, ql]
    return max(int(rng.choice(pool)), 1)


def dress(rng, vec, unwanted=False, high=False):
    """The regions of a read with pass A's fields: scores around T (all under it: unwanted), a seed coverage, for about a third a
    lower-scoring copy over the same interval, the whole in a random order."""
    out = []
    for a in vec:
        a = a.copy()
        ql = int(a["qe"]) - int(a["qb"])
        a["score"] = int(rng.integers(5, T)) if unwanted else _score(rng, ql, high)
        a["seedcov"], a["csub"] = int(rng.integers(19, max(ql, 20) + 1)), int(rng.choice([0, 0, 0, 20]))
        out.append(a)
        if rng.random() < 0.35:
            b, s = a.copy(), int(a["score"])
            b["score"] = max(int(rng.choice([s - 1, s - 1, (3 * s) // 4, s // 2 - 1])), 1)
            out.append(b)
    if not out:
        return np.zeros(0, dtype=kswlib.ALNREG)
    return np.array(out, dtype=kswlib.ALNREG)[rng.permutation(len(out))]


def filler(rng, whole):
    """a read with one region that any pass A wants"""
    seg, rb, re, truesc, w = wg.segment(rng, whole, "exact", 80)
    a = wg.region(0, len(seg), rb, re, truesc, w, len(seg))
    a["seedcov"] = len(seg) // 2
    return seg, np.array([a], dtype=kswlib.ALNREG)


def se_slice(rng, whole, n_reads):
    """-> (reads, vectors): every fifth read without a region, every seventh with regions all under T"""
    reads, vectors, _ = wg.random_slice(rng, whole, n_reads)
    return reads, [dress(rng, v, unwanted=i % 7 == 3) for i, v in enumerate(vectors)]


def _mate(rng, whole, pos, ln, rev):
    src = whole[pos:pos + ln]
    one = [(int(rng.integers(5, ln - 5)), int(rng.choice([-2, -1, 1, 2])))] if rng.random() < 0.4 else []
    seg = wg.edit(rng, src, int(rng.integers(0, 4)), one)
    rb, re = wg.on_strand(pos, pos + ln, rev)
    return (wg.revcomp(seg) if rev else seg), wg.region(0, len(seg), rb, re, min(len(seg), ln) - 14 - int(rng.integers(0, 30)), 100)


def _end(rng, whole, bases, reg, high):
    """one end of a pair: its placed region, for some a chimeric segment elsewhere behind it, dressed"""
    regs = [reg]
    if rng.random() < 0.3:
        rev = bool(rng.integers(0, 2))
        seg, rb, re, truesc, w = wg.segment(rng, whole, wg.KINDS[int(rng.integers(0, len(wg.KINDS)))], int(rng.integers(30, 120)))
        rb, re = wg.on_strand(rb, re, rev)
        regs.append(wg.region(len(bases), len(bases) + len(seg), rb, re, truesc, w))
        bases = np.concatenate([bases, wg.revcomp(seg) if rev else seg])
    return bases, dress(rng, regs, high=high)


def pe_slice(rng, whole, n_pairs):
    """-> (reads, vectors), 2 * n_pairs of each.  Of ten pairs six are FR at an insert the model likes with good scores, one is FR
    with scores as they come, one lies too far apart, one has its ends in two sequences or on one strand, one has an empty end."""
    reads, vectors = [], []
    for p in range(n_pairs):
        kind = p % 10
        off, n = wg.CONTIGS[int(rng.choice([0, 0, 0, 1, 1, 2]))]
        l0, l1 = int(rng.integers(50, 110)), int(rng.integers(50, 110))
        if kind == 7:  # 1500 to 2500 bases apart in the longest sequence
            off, n = wg.CONTIGS[0]
            ins = int(rng.integers(1500, 2500))
        else:
            ins = int(np.clip(rng.normal(300, 80), 130, min(600, n - 30)))
        pos0 = off + int(rng.integers(5, n - ins - 5))
        pos1 = pos0 + ins - l1
        rev1 = True
        if kind == 8:
            if p % 20 == 8:  # the mate in another sequence
                off2, n2 = wg.CONTIGS[1 if off == 0 else 0]
                pos1 = off2 + int(rng.integers(5, n2 - l1 - 5))
            else:            # both forward: FF is not open
                rev1 = False
        b0, r0 = _mate(rng, whole, pos0, l0, False)
        b1, r1 = _mate(rng, whole, pos1, l1, rev1)
        ends = [_end(rng, whole, b0, r0, kind < 6), _end(rng, whole, b1, r1, kind < 6)]
        if kind == 9:
            ends[p // 10 % 2] = (kswgen.rand_seq(rng, 60), np.zeros(0, dtype=kswlib.ALNREG))
        if rng.random() < 0.3:  # the reverse read first
            ends.reverse()
        for b, v in ends:
            reads.append(b), vectors.append(v)
    return reads, vectors


def decide(o, pes, id0, vectors):
    return load_package().decide_batch(o, wg.L_PAC, pes, id0, vectors)


def exact(rng, whole, o, pes, id0, reads, vectors, n_wanted):
    """The longest prefix of the slice (in reads, or pairs) whose wanted regions do not pass n_wanted, filled up with reads of one
    wanted region each (paired-end: with an empty mate).  -> (reads, vectors) with exactly n_wanted wanted regions."""
    step = 2 if int(o["flag"]) & PE else 1
    nw = decide(o, pes, id0, vectors)["n_want"]
    keep, have = 0, 0
    for u in range(0, len(vectors), step):
        m = int(nw[u:u + step].sum())
        if have + m > n_wanted:
            break
        keep, have = u + step, have + m
    reads, vectors = list(reads[:keep]), list(vectors[:keep])
    while have < n_wanted:
        b, v = filler(rng, whole)
        reads.append(b), vectors.append(v)
        if step == 2:
            reads.append(kswgen.rand_seq(rng, 60)), vectors.append(np.zeros(0, dtype=kswlib.ALNREG))
        have += 1
    assert int(decide(o, pes, id0, vectors)["n_want"].sum()) == n_wanted
    return reads, vectors


def make(mode, n_wanted=None, units=None, w=100, seed=0):
    """A slice by its number of wanted regions or of units.  mode: "se", "se-all", "pe", "pe-all".  -> (o, pes, id0, reads, vectors)"""
    pe = mode.startswith("pe")
    o, pes, id0 = opt(w, (PE if pe else 0) | (ALL if mode.endswith("all") else 0)), (pes_fr() if pe else None), 7000
    rng = np.random.default_rng([seed, n_wanted or 0, units or 0, int(pe)])
    whole, _ = wg.reference()
    n = units if units is not None else max(n_wanted, 4) * (2 if pe else 3)  # (generous: about one wanted region per read)
    reads, vectors = pe_slice(rng, whole, n) if pe else se_slice(rng, whole, n)
    if n_wanted is not None:
        reads, vectors = exact(rng, whole, o, pes, id0, reads, vectors, n_wanted)
    return o, pes, id0, reads, vectors


def _key(a):
    return tuple(int(a[k]) for k in ("rb", "re", "qb", "qe", "score", "truesc", "w"))


def shapes(o, vectors, host):
    """what a slice contains, from the vectors as given and as bmh_decide_batch left them"""
    s = dict(no_region=0, none_wanted=0, moved_first=0, multi_secondary=0, paired=0, unpaired=0)
    for v, a, ks in zip(vectors, host["regs"], host["want"]):
        s["no_region"] += len(v) == 0
        s["none_wanted"] += len(v) > 0 and len(ks) == 0
        if len(ks):
            s["moved_first"] += _key(v[int(ks[0])]) != _key(a[int(ks[0])])
            s["multi_secondary"] += len(ks) >= 2 and any(int(a[int(k)]["secondary"]) >= 0 for k in ks)
    if int(o["flag"]) & PE:
        s["paired"] = int((host["pd"]["paired"] != 0).sum())
        s["unpaired"] = len(host["pd"]) - s["paired"]
    s["total"], s["n_w"] = sum(len(v) for v in vectors), int(host["n_want"].sum())
    return s
