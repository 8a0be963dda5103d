#!/usr/bin/env python3
"""Fixture for the stage-to-stage tests (tests/pipechain.py, tests/test_pipeline_chain_*.py): one chunk of reads, paired-end and
single-end, through the COMPILED REFERENCE's `bwa mem -t 1` (oracle/_ref/bwa, run as a plain child process, the project's shim not
in front of it) under two option sets, on a 48 kb genome of three contigs with repeat families and tandem duplications.
Stored (data only): the genome's base codes and contig table, the index arrays as reflib.bwt_arrays returns them, the packed
reference, the reads with names and qualities, per run the mem_opt_t fields and the SAM body (the @ lines dropped) with per-read
offsets, and the counts of the read shapes the reference's own output contains -- asserted here against their minimums before
anything is written.
Output: tests/golden/pipeline_golden.npz.  Run in the build container: python tools/make_pipeline_fixture.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kswgen  # noqa: E402
import reflib  # noqa: E402

CONTIGS = (("ctgA", 21000), ("ctgB", 9000), ("ctgC", 18000))
RUNS = ("pe0", "se0", "pe1", "se1")
OPTION_ARGS = ([], ["-A", "2", "-B", "5", "-w", "12", "-r", "1.2"])
# the scalar fields of mem_opt_t (bwamem.h:21-48) the package's option records are made from
OPT_INT = ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_unpaired", "pen_clip5", "pen_clip3", "w", "zdrop", "T", "flag", "min_seed_len",
           "split_width", "max_occ", "max_chain_gap", "mapQ_coef_fac", "max_ins", "max_matesw")
OPT_FLOAT = ("split_factor", "mask_level", "chain_drop_ratio", "mask_level_redun", "mapQ_coef_len")
OPT_REC = np.dtype([(k, "<i4") for k in OPT_INT] + [(k, "<f4") for k in OPT_FLOAT] + [("mat", "i1", (25,))])
MEM_F_PE = 0x2
# what the reference's SAM of a run must hold at least, by shape (pe: the paired-end runs, se: the single-end runs).  Neither option
# set has -a or -M, so the reference prints no line with flag 0x100: the secondaries of the repeat reads show as mapQ 0 and XS > 0.
MINIMUM = {"reverse": 40, "forward": 40, "first_base": 1, "last_base": 1, "straddle": 2, "with_n": 4, "error_free": 15, "mapq0": 8, "xs": 20,
           "flag_0x100": 0, "unmapped": 5, "flag_0x800": 3, "sa_tag": 6, "soft_clip": 8, "long_cigar": 1, "reads_250": 3}
MINIMUM_PE = {"rescued": 10, "proper": 120, "improper": 4}
MUT_TAG = b"mut"  # in the name of a pair whose mate no seed can place


def rc(s):
    s = np.asarray(s, dtype=np.uint8)[::-1]
    return np.where(s < 4, 3 - s, 4).astype(np.uint8)


def build_genome(rng):
    total = sum(n for _, n in CONTIGS)
    ref = kswgen.rand_seq(rng, total)
    offs = np.concatenate([[0], np.cumsum([n for _, n in CONTIGS])]).astype(np.int64)
    taken = [(int(o) - 400, int(o) + 400) for o in offs]  # contig boundaries and the genome's ends stay unique sequence

    def place(length):
        while True:
            at = int(rng.integers(400, total - 400 - length))
            if all(at + length + 60 <= lo or at >= hi + 60 for lo, hi in taken):
                taken.append((at, at + length))
                return at
    fams = []
    for copies, div in ((3, 0.0), (5, 0.01), (8, 0.02), (12, 0.04)):  # repeat families
        length = int(rng.integers(220, 420))
        src = kswgen.rand_seq(rng, length + 40)
        locs = []
        for _ in range(copies):
            at = place(length)
            ref[at:at + length] = kswgen.mutate(rng, src, div, 0.001 if div else 0.0, 0.001 if div else 0.0, 2)[:length]
            locs.append((at, length))
        fams.append(locs)
    sites = []
    for _ in range(3):  # tandem duplications
        P = int(rng.integers(25, 41))  # noqa: N806
        at = place(2 * P + 200) + 100
        ref[at + P:at + 2 * P] = ref[at:at + P]
        sites.append((at, P))
    return np.ascontiguousarray(ref, dtype=np.uint8), offs, fams, sites, taken


def write_fasta(path, ref, offs):
    with open(path, "w") as f:
        for (name, n), o in zip(CONTIGS, offs):
            f.write(f">{name}\n")
            s = "".join("ACGT"[c] for c in ref[int(o):int(o) + n])
            for i in range(0, n, 70):
                f.write(s[i:i + 70] + "\n")


class World:
    def __init__(self, rng, ref, offs, fams, sites, taken):
        self.rng, self.ref, self.offs, self.fams, self.sites, self.taken = rng, ref, offs, fams, sites, taken
        self.total = len(ref)

    def length(self):
        return int(self.rng.integers(70, 151))

    def unique_pos(self, span):
        """the start of `span` bases inside one contig that touch no repeat copy, duplication or boundary zone"""
        while True:
            at = int(self.rng.integers(0, self.total - span))
            if all(at + span <= lo or at >= hi for lo, hi in self.taken):
                return at

    def light(self, s, n):
        return kswgen.mutate(self.rng, s, 0.015, 0.002, 0.002, 2)[:n]

    def spaced(self, s):
        """a substitution every 5 to 10 bases (about 13 %): no exact run reaches min_seed_len, so only mate rescue places the read"""
        s = s.copy()
        i = int(self.rng.integers(2, 6))
        while i < len(s):
            s[i] = (int(s[i]) + int(self.rng.integers(1, 4))) & 3
            i += int(self.rng.integers(5, 11))
        return s

    def many_indels(self, at):
        """250 bases: 46 bases for the seeds, then 12 single-base deletions and insertions in turn, 17 bases apart"""
        ref, parts = self.ref, [self.ref[at:at + 46]]
        at += 46
        for j in range(12):
            if j % 2:
                parts.append(np.array([next(x for x in range(4) if x != ref[at - 1] and x != ref[at])], dtype=np.uint8))  # unlike both neighbours
            else:
                at += 1
            parts.append(ref[at:at + 17])
            at += 17
        rd = np.concatenate(parts)
        return rd[:250] if len(rd) >= 250 else np.concatenate([rd, ref[at:at + 250 - len(rd)]])


def single_reads(w):
    """(name, codes) per read: the single-end set"""
    rng, ref, out = w.rng, w.ref, []

    def add(tag, s, flip=None):
        if flip if flip is not None else rng.random() < 0.5:
            s = rc(s)
        out.append((tag, np.ascontiguousarray(s, dtype=np.uint8)))
    for _ in range(66):
        n = w.length()
        at = w.unique_pos(n + 20)
        add("plain", w.light(ref[at:at + n + 20], n))
    for flip in (False, True):  # the first and the last base of the genome, the ends of two contigs
        add("first", ref[:100 + 17 * flip].copy(), flip)
        add("last", ref[w.total - 120 + 9 * flip:].copy(), flip)
    for b in w.offs[1:-1]:  # across a contig boundary
        for k, flip in enumerate((False, True, False)):
            lo = int(b) - (60, 35, 100)[k]
            add("straddle", ref[lo:lo + 130].copy(), flip)
    for _ in range(10):
        n = w.length()
        at = w.unique_pos(n)
        s = w.light(ref[at:at + n + 20], n)
        s[int(rng.integers(0, n))] = 4
        if rng.random() < 0.3:
            k = int(rng.integers(0, n - 4))
            s[k:k + 3] = 4
        add("n", s)
    for _ in range(20):
        n = w.length()
        at = w.unique_pos(n)
        add("exact", ref[at:at + n].copy())
    for k in range(40):  # from repeat copies, inside and over their edges
        locs = w.fams[k % len(w.fams)]
        at, length = locs[int(rng.integers(0, len(locs)))]
        n = int(rng.integers(70, 131))
        pos = at + (int(rng.integers(0, length - n)) if k % 3 else int(rng.integers(-n // 2, length - n // 2)))
        s = ref[pos:pos + n + 20]
        add("rep", s[:n].copy() if k % 2 else w.light(s, n))
    for k in range(6):  # across a tandem duplication, with a copy more or less than the genome has
        at, P = w.sites[k % len(w.sites)]  # noqa: N806
        add("tandem", np.concatenate([ref[at - 50:at]] + [ref[at:at + P]] * (1 if k % 2 else 3) + [ref[at + 2 * P:at + 2 * P + 50]]))
    for _ in range(10):
        add("random", kswgen.rand_seq(rng, w.length()), False)
    for k in range(10):  # chimeric: two stretches from different places
        a, b = w.unique_pos(80), w.unique_pos(80)
        la, lb = int(rng.integers(60, 76)), int(rng.integers(60, 76))
        add("chimera", np.concatenate([ref[a:a + la], rc(ref[b:b + lb]) if k % 2 else ref[b:b + lb]]))
    for k in range(12):  # one long deletion or insertion near an end
        n = int(rng.integers(110, 151))
        at = w.unique_pos(n + 40)
        cut, gap = int(rng.integers(14, 22)), int(rng.integers(16, 28))
        if k % 2:
            s = np.concatenate([ref[at:at + n - cut], ref[at + n - cut + gap:at + n + gap]])
        else:
            s = np.concatenate([ref[at:at + cut], kswgen.rand_seq(rng, gap), ref[at + cut:at + n - gap]])
        add("endgap", s)
    for k in range(6):  # 250 bases
        at = w.unique_pos(300)
        add("long" if k >= 2 else "longcigar", w.light(ref[at:at + 270], 250) if k >= 2 else w.many_indels(at), bool(k & 1))
    order = rng.permutation(len(out))
    return [(b"s%d:%s" % (i, out[j][0].encode()), out[j][1]) for i, j in enumerate(order)]


def paired_reads(w):
    """(name, codes of read 1, codes of read 2) per pair: the paired-end set"""
    rng, ref, out = w.rng, w.ref, []

    def fr(n1, n2, unique=True, at=None):
        """an FR pair's two stretches, insert 300 +- 60: (forward stretch, reverse-complemented stretch)"""
        d = int(np.clip(rng.normal(300, 60), max(n1, n2) + 5, 520))
        if at is None:
            at = w.unique_pos(d) if unique else int(rng.integers(0, w.total - d))
        return ref[at:at + n1].copy(), rc(ref[at + d - n2:at + d])

    def add(tag, m1, m2):
        if rng.random() < 0.5:
            m1, m2 = m2, m1
        out.append((tag, np.ascontiguousarray(m1, dtype=np.uint8), np.ascontiguousarray(m2, dtype=np.uint8)))
    for _ in range(80):
        n1, n2 = w.length(), w.length()
        a, b = fr(n1 + 20, n2 + 20)
        add("plain", w.light(a, n1), rc(w.light(rc(b), n2)))
    for _ in range(18):
        add("exact", *fr(w.length(), w.length()))
    for k in range(30):  # a mate no seed places
        n1, n2 = int(rng.integers(90, 151)), int(rng.integers(125, 151))
        a, b = fr(n1, n2)
        out.append((MUT_TAG.decode(), a, w.spaced(b)) if k % 2 else (MUT_TAG.decode(), w.spaced(rc(b)), rc(a)))
    for k in range(20):  # read 1 inside a repeat copy
        locs = w.fams[k % len(w.fams)]
        at, length = locs[int(rng.integers(0, len(locs)))]
        n1, n2 = int(rng.integers(70, 121)), w.length()
        a, b = fr(n1, n2, at=at + int(rng.integers(0, length - n1)))
        add("rep", a, b)
    for k in range(12):  # both mates inside one copy of the families with the least divergence: mapQ 0
        at, length = w.fams[k % 2][int(rng.integers(0, len(w.fams[k % 2])))]
        n1, n2 = int(rng.integers(70, 101)), int(rng.integers(70, 101))
        add("rep2", ref[at + k:at + k + n1].copy(), rc(ref[at + length - n2 - k:at + length - k]))
    add("first", ref[:110].copy(), rc(ref[200:310]))  # the genome's first and last base, and pairs across the contig boundaries
    add("last", ref[w.total - 320:w.total - 200].copy(), rc(ref[w.total - 95:]))
    for b in w.offs[1:-1]:
        add("straddle", ref[int(b) - 280:int(b) - 160].copy(), rc(ref[int(b) - 50:int(b) + 70]))
        add("straddle", ref[int(b) - 40:int(b) + 90].copy(), rc(ref[int(b) + 180:int(b) + 290]))
    for k in range(4):
        at, P = w.sites[k % len(w.sites)]  # noqa: N806
        m1 = np.concatenate([ref[at - 50:at]] + [ref[at:at + P]] * (1 if k % 2 else 3) + [ref[at + 2 * P:at + 2 * P + 50]])
        add("tandem", m1, rc(ref[at + 200:at + 300]))
    for k in range(10):  # no proper pair: both mates forward, or on different contigs, or far apart
        n = w.length()
        a, b = w.unique_pos(n), w.unique_pos(n)
        add("apart", ref[a:a + n].copy(), ref[b:b + n].copy() if k % 2 else rc(ref[b:b + n]))
    for _ in range(6):
        add("random", kswgen.rand_seq(rng, w.length()), kswgen.rand_seq(rng, w.length()))
    for _ in range(6):
        n1, n2 = w.length(), w.length()
        a, b = fr(n1, n2)
        a[int(rng.integers(0, n1))] = 4
        add("n", a, b)
    for k in range(4):  # a chimeric read with an ordinary mate
        x = w.unique_pos(80)
        a, b = fr(70, w.length())
        add("chimera", np.concatenate([a, rc(ref[x:x + 66]) if k % 2 else ref[x:x + 66]]), b)
    for k in range(4):
        at = w.unique_pos(560)
        m1 = w.many_indels(at) if k < 2 else w.light(ref[at:at + 270], 250)
        add("longcigar" if k < 2 else "long", m1, rc(ref[at + 300:at + 550]))
    order = rng.permutation(len(out))
    return [(b"p%d:%s" % (i, out[j][0].encode()), out[j][1], out[j][2]) for i, j in enumerate(order)]


def quality(i, n):
    """a quality string that compresses: a ramp whose phase depends on the read"""
    return bytes(35 + (i * 5 + j // 4) % 38 for j in range(n))


def letters(codes):
    return "".join("ACGTN"[c] for c in codes)


def mem_options(args, pe):
    """mem_opt_t as `bwa mem` leaves it for these arguments (fastmap.c:40-157): mem_opt_init, the options, -A's scaling"""
    L = reflib.lib()  # noqa: N806
    o = L.mem_opt_init().contents
    given = set()
    for k, v in zip(args[::2], args[1::2]):
        field = {"-A": "a", "-B": "b", "-w": "w", "-r": "split_factor"}[k]
        setattr(o, field, float(v) if field == "split_factor" else int(v))
        given.add(field)
    if "a" in given:
        for f in ("b", "T", "o_del", "e_del", "o_ins", "e_ins", "zdrop", "pen_clip5", "pen_clip3", "pen_unpaired"):
            if f not in given:
                setattr(o, f, getattr(o, f) * o.a)
    L.bwa_fill_scmat(o.a, o.b, o.mat)
    if pe:
        o.flag |= MEM_F_PE
    rec = np.zeros((), dtype=OPT_REC)
    for f in OPT_INT + OPT_FLOAT:
        rec[f] = getattr(o, f)
    rec["mat"] = [o.mat[i] for i in range(25)]
    return rec


def run_mem(fa, args, files):
    """the SAM body of the reference's `bwa mem -t 1`, a child process in this one's environment: the project's shim is not in front"""
    assert "libbwamem_hip" not in os.environ.get("LD_PRELOAD", "")
    p = subprocess.run([reflib.REF_BWA, "mem", "-t", "1", "-v", "1"] + args + [fa] + files, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    return b"".join(ln for ln in p.stdout.splitlines(keepends=True) if not ln.startswith(b"@"))


def split_by_read(body, names, pe):
    """n + 1 offsets into the SAM body: the lines of read i, in read order (mates: read 1's lines, then read 2's)"""
    off, at, i = [0], 0, 0
    for ln in body.splitlines(keepends=True):
        f = ln.split(b"\t")
        k = int(f[0][1:f[0].index(b":")])
        r = 2 * k + (1 if int(f[1]) & 0x80 else 0) if pe else k
        assert names[r] == f[0] and r >= i, (r, i, f[0])
        while i < r:
            off.append(at)
            i += 1
        at += len(ln)
    while i < len(names):
        off.append(at)
        i += 1
    assert len(off) == len(names) + 1 and off[-1] == len(body)
    return np.array(off, dtype=np.int64)


def count_shapes(body, pe, total, offs):
    """the shapes of MINIMUM (and MINIMUM_PE), counted on a SAM body alone; tests/test_pipeline_chain_cpu.py counts them again"""
    c = dict.fromkeys(list(MINIMUM) + (list(MINIMUM_PE) if pe else []), 0)
    bounds = [int(o) for o in offs[1:-1]]
    lens = {n.encode(): ln for n, ln in CONTIGS}
    start = {n.encode(): int(o) for (n, _), o in zip(CONTIGS, offs)}
    for ln in body.splitlines():
        f = ln.split(b"\t")
        flag, mapq, cigar, seq = int(f[1]), int(f[4]), f[5], f[9]
        tags = {t[:2]: t[5:] for t in f[11:]}
        c["flag_0x100"] += bool(flag & 0x100)
        c["flag_0x800"] += bool(flag & 0x800)
        c["sa_tag"] += b"SA" in tags
        if flag & 0x4:
            c["unmapped"] += 1
            continue
        c["reverse" if flag & 0x10 else "forward"] += 1
        ops, at = [], 0
        for i, ch in enumerate(cigar):
            if ch in b"MIDNSHP=X":
                ops.append((int(cigar[at:i]), chr(ch)))
                at = i + 1
        span = sum(n for n, ch in ops if ch in "MD")
        pos = start[f[2]] + int(f[3]) - 1
        c["first_base"] += pos == 0
        c["last_base"] += pos + span == total
        c["straddle"] += (pos in bounds and ops[0][1] == "S") or (pos + span in bounds and ops[-1][1] == "S")  # clipped at a contig's edge
        c["with_n"] += b"N" in seq
        c["error_free"] += int(tags.get(b"NM", b"1")) == 0 and len(ops) == 1
        c["mapq0"] += mapq == 0
        c["xs"] += int(tags.get(b"XS", b"0")) > 0
        c["soft_clip"] += b"S" in cigar
        c["long_cigar"] += len(ops) > 24
        c["reads_250"] += len(seq) == 250 and not flag & 0x800
        if pe:
            c["proper"] += bool(flag & 0x2) and not flag & 0x900
            c["improper"] += not flag & 0x2 and not flag & 0x908
            c["rescued"] += bool(flag & 0x2) and not flag & 0x900 and MUT_TAG in f[0] and bool(flag & 0x40)
        assert pos + span <= start[f[2]] + lens[f[2]]
    return c


def main():
    assert reflib.have_ref_bwa(), "oracle/_ref is not built"
    rng = np.random.default_rng(20261020)
    ref, offs, fams, sites, taken = build_genome(rng)
    w = World(rng, ref, offs, fams, sites, taken)
    tmp = tempfile.mkdtemp(prefix="bmh_pipeline_")
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, ref, offs)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac, pac = reflib.pac_of(idx)
    assert l_pac == len(ref)
    prim, L2, seq_len, words, sa_intv, sa = reflib.bwt_arrays(idx)  # noqa: N806
    out = {"genome": ref, "contig_names": np.array([n for n, _ in CONTIGS]), "contig_off": offs[:-1].copy(), "contig_len": np.array([n for _, n in CONTIGS], dtype=np.int64),
           "l_pac": np.int64(l_pac), "pac": pac, "bwt_primary": np.uint64(prim), "bwt_L2": np.array(L2, dtype=np.uint64), "bwt_seq_len": np.uint64(seq_len),
           "bwt_words": words, "bwt_sa_intv": np.int32(sa_intv), "bwt_sa": sa, "runs": np.array(RUNS)}
    se, pe = single_reads(w), paired_reads(w)
    sets = {"se": ([n for n, _ in se], [s for _, s in se], None),
            "pe": ([n for n, _, _ in pe for _k in (0, 1)], [s for _, a, b in pe for s in (a, b)], True)}
    files = {}
    for key, (names, reads, qual) in sets.items():
        quals = [quality(i, len(r)) for i, r in enumerate(reads)] if qual else None
        out[key + "_names"], out[key + "_reads"] = np.array(names), np.concatenate(reads)
        out[key + "_read_len"] = np.array([len(r) for r in reads], dtype=np.int32)
        if quals:
            out[key + "_qual"] = np.frombuffer(b"".join(quals), dtype=np.uint8)
        if key == "se":  # FASTA: no qualities
            files[key] = [os.path.join(tmp, "se.fa")]
            with open(files[key][0], "w") as f:
                for n, r in zip(names, reads):
                    f.write(">" + n.decode() + "\n" + letters(r) + "\n")
        else:
            files[key] = [os.path.join(tmp, "pe_1.fq"), os.path.join(tmp, "pe_2.fq")]
            for m in (0, 1):
                with open(files[key][m], "w") as f:
                    for i in range(m, len(reads), 2):
                        f.write("@" + names[i].decode() + "\n" + letters(reads[i]) + "\n+\n" + quals[i].decode() + "\n")
    for run in RUNS:
        key, args = run[:2], OPTION_ARGS[int(run[2])]
        names = sets[key][0]
        body = run_mem(fa, args, files[key])
        assert body == run_mem(fa, args, files[key]), run  # the reference repeats itself
        off = split_by_read(body, names, key == "pe")
        assert (np.diff(off) > 0).all(), run  # every read has a line
        counts = count_shapes(body, key == "pe", len(ref), offs)
        need = {**MINIMUM, **(MINIMUM_PE if key == "pe" else {})}
        short = {k: (counts[k], v) for k, v in need.items() if counts[k] < v}
        print(run, len(names), "reads,", body.count(b"\n"), "lines,", len(body), "bytes:", counts)
        assert not short, (run, short)
        out[run + "_opt"] = mem_options(args, key == "pe")
        out[run + "_sam"], out[run + "_sam_off"] = np.frombuffer(body, dtype=np.uint8), off
        out[run + "_shape_names"], out[run + "_shape_counts"] = np.array(sorted(counts)), np.array([counts[k] for k in sorted(counts)], dtype=np.int32)
    path = os.path.join(ROOT, "tests", "golden", "pipeline_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 512332


if __name__ == "__main__":
    main()
