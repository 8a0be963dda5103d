"""Constructed slices for pass C of phase 2 (bmh_sam_text_batch / bmh_sam_text_device).  The text call never reads a base of the
reference, so the records are not real alignments: a CIGAR only has to consume its query interval and lie inside one sequence.  What
a slice holds is pass A's and pass B's outputs as the call takes them -- vectors, the want list, pair decisions, mapQs, records and the
two pools -- made directly, so that every shape the text can take is there on purpose: see make() and shapes()."""
import ctypes as C

import numpy as np

import kswlib
from __graft_entry__ import load_package

T = 30
PE, NOPAIRING, ALL, NO_MULTI = 0x2, 0x4, 0x8, 0x10
# a sequence table with a 2 x 10^9-base sequence, names of 1 and 250 bytes, and l_pac past 2^32 (so reverse-strand coordinates pass 2^33)
CONTIGS = [(0, 5000), (5000, 2_000_000_123), (2_000_005_123, 9), (2_000_005_132, 2_147_000_000), (4_147_005_132, 40_000),
           (4_147_045_132, 500_000_000)]  # (a sequence's length is an int32: bntann1_t)
NAMES = [b"chr1", b"big|2e9", b"c", b"Q" * 250, b"chrUn_KI270442v1", b"chrZ"]
assert all(n < 1 << 31 for _, n in CONTIGS) and all(CONTIGS[i][0] + CONTIGS[i][1] == CONTIGS[i + 1][0] for i in range(len(CONTIGS) - 1))
L_PAC = CONTIGS[-1][0] + CONTIGS[-1][1]
assert L_PAC > 1 << 32
EDGES = [0, 8, 9, 98, 99, 998, 999, 9_998, 9_999, 99_998, 99_999, 999_998, 999_999, 9_999_998, 9_999_999, 99_999_998, 99_999_999,
         999_999_998, 999_999_999, 1_999_999_999]  # 0-based positions on both sides of every digit count of POS


def refidx():
    return load_package().make_refidx([(o, n) for o, n in CONTIGS], L_PAC, NAMES)


def sam_opt(flag=0):
    pkg = load_package()
    o = np.zeros((), dtype=pkg.SAM_OPT)
    o["a"], o["b"], o["o_del"], o["e_del"], o["o_ins"], o["e_ins"], o["pen_unpaired"], o["w"] = 1, 4, 6, 1, 6, 1, 17, 100
    o["T"], o["flag"], o["min_seed_len"], o["max_ins"], o["mapQ_coef_fac"], o["max_matesw"] = T, flag, 19, 10000, 0, 100
    o["mask_level"], o["mask_level_redun"], o["mapQ_coef_len"] = 0.5, 0.95, 50
    return o


def pes_fr():
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    pes["failed"] = 1
    pes[1]["failed"], pes[1]["low"], pes[1]["high"], pes[1]["avg"], pes[1]["std"] = 0, 50, 800, 300.0, 80.0
    return pes


def _edge(rng):
    """a small number on either side of a digit count"""
    return int(rng.choice([0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]))


def _cigar(rng, ql, kind):
    """M / I / D runs that consume ql query bases; kind: "plain", "lead" (a leading deletion), "trail" (a trailing one)"""
    words, left = [], ql
    if kind == "lead":
        words.append(int(rng.integers(1, 12)) << 4 | 2)
    first = True
    while left > 0:
        op = 0 if first or left < 3 else int(rng.choice([0, 0, 0, 1, 2]))
        if words and words[-1] & 0xf == op:
            op = 0 if op else 1
        ln = int(rng.integers(1, 60))
        if op != 2:
            ln = min(ln, left)
            left -= ln
        words.append(ln << 4 | op)
        first = False
    if words[-1] & 0xf == 2:
        words.pop()
    if kind == "trail":
        words.append(int(rng.integers(1, 12)) << 4 | 2)
    return words


def _md(rng):
    n = int(rng.integers(0, 6))
    s = b"%d" % _edge(rng)
    for _ in range(n):
        s += (b"^" if rng.random() < 0.3 else b"") + bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 4))).tolist()) + b"%d" % int(rng.integers(0, 150))
    return s


class Builder:
    def __init__(self, rng, flag):
        self.rng, self.flag = rng, flag
        self.seqs, self.vectors, self.want, self.mapq, self.res, self.cig, self.md, self.pd = [], [], [], [], [], [], bytearray(), []
        self.n_reads = 0

    def read(self, l_seq=None, name=None, qual=True, comment=False):
        rng = self.rng
        l_seq = int(rng.integers(30, 301)) if l_seq is None else l_seq
        seq = rng.integers(0, 5, l_seq).astype(np.uint8)
        q = bytes(rng.integers(33, 74, l_seq).astype(np.uint8).tolist()) if qual else None
        name = name if name is not None else b"read%d" % (self.n_reads // 2 if self.flag & PE else self.n_reads)
        com = (b"BC:Z:%d" % self.n_reads if self.n_reads % 3 else b"") if comment else None
        self.n_reads += 1
        return (name, com, seq, q)

    def region(self, l_seq, where=None, rev=None, clip=None, kind="plain", secondary=-1, score=None, pool=True):
        """-> (ALNREG record, WANTED_RES record) of a region of a read of l_seq bases; where: (contig, 0-based leftmost forward base);
        pool=False: a region nobody prints, nothing goes into the pools"""
        rng = self.rng
        clip = clip if clip is not None else str(rng.choice(["none", "5", "3", "both"]))
        rev = bool(rng.integers(0, 2)) if rev is None else rev
        c5 = int(rng.integers(1, max(l_seq // 3, 2))) if clip in ("5", "both") and l_seq > 3 else 0
        c3 = int(rng.integers(1, max(l_seq // 3, 2))) if clip in ("3", "both") and l_seq > 3 else 0
        qb, qe = (c3, l_seq - c5) if rev else (c5, l_seq - c3)  # the clips are named by the printed strand
        words = _cigar(rng, qe - qb, kind)
        tl = sum(w >> 4 for w in words if w & 0xf in (0, 2))
        if where is None:
            ci = int(rng.integers(0, len(CONTIGS)))
            ci = ci if CONTIGS[ci][1] >= tl else 0
            where = (ci, int(rng.integers(0, CONTIGS[ci][1] - tl + 1)))
        ci, p = where
        p = min(p, CONTIGS[ci][1] - tl)
        lead = words[0] >> 4 if words[0] & 0xf == 2 else 0
        b = CONTIGS[ci][0] + p - lead if p >= lead else CONTIGS[ci][0]  # (POS is past a leading deletion: keep it at p where it fits)
        rb, re = (2 * L_PAC - (b + tl), 2 * L_PAC - b) if rev else (b, b + tl)
        a = np.zeros((), dtype=kswlib.ALNREG)
        a["rb"], a["re"], a["qb"], a["qe"], a["secondary"] = rb, re, qb, qe, secondary
        a["score"] = score if score is not None else T + _edge(rng)
        a["truesc"], a["sub"], a["csub"], a["w"], a["seedcov"] = a["score"], _edge(rng) if rng.random() < 0.7 else 0, _edge(rng) if rng.random() < 0.3 else 0, 100, 20
        x = np.zeros((), dtype=load_package().WANTED_RES)
        x["rb"], x["re"], x["qb"], x["qe"], x["score"], x["n_cigar"], x["NM"], x["tries"] = rb, re, qb, qe, a["score"], len(words), _edge(rng), 1
        m = _md(rng)
        x["cigar_off"], x["md_off"], x["md_len"] = len(self.cig), len(self.md), len(m)
        if pool:
            self.cig += words
            self.md += m + b"\0"
        return a, x

    def add(self, s, regs, n_junk=0):
        """a read, its wanted regions [(ALNREG, WANTED_RES)] in want order -- the first one is region 0 -- and junk regions under T between them"""
        rng = self.rng
        vec, ks = [], []
        for a, x in regs:
            ks.append(len(vec))
            vec.append(a)
            self.res.append(x)
            for _ in range(n_junk):
                j = a.copy()
                j["score"], j["secondary"] = int(rng.integers(1, T)), -1
                vec.append(j)
        if not regs and n_junk:
            vec.append(self.region(len(s[2]), score=T - 1, pool=False)[0])
        self.seqs.append(s), self.want.append(np.array(ks, dtype=np.int32))
        self.vectors.append(np.array(vec, dtype=kswlib.ALNREG).reshape(-1) if vec else np.zeros(0, dtype=kswlib.ALNREG))
        mq = rng.integers(0, 61, len(vec)).astype(np.int32)
        if len(ks) >= 2 and rng.random() < 0.6:
            mq[ks[0]] = int(rng.integers(0, 20))  # the cap bites: a later line's mapQ is above the first's
        self.mapq.append(mq)

    def done(self, rg_id):
        pkg = load_package()
        roff = np.concatenate([[0], np.cumsum([len(v) for v in self.vectors])]).astype(np.int64)
        want_k = np.full(int(roff[-1]) + 1, -1, dtype=np.int32)
        for i, ks in enumerate(self.want):
            want_k[int(roff[i]):int(roff[i]) + len(ks)] = ks
        dec = {"pd": np.array(self.pd, dtype=pkg.PAIRDEC).reshape(-1) if self.pd else np.zeros(0, dtype=pkg.PAIRDEC),
               "reg_mapq": np.concatenate(self.mapq + [np.zeros(1, dtype=np.int32)]).astype(np.int32),
               "n_want": np.array([len(k) for k in self.want], dtype=np.int32), "want_k": want_k, "want": self.want}
        res = np.array(self.res, dtype=pkg.WANTED_RES).reshape(-1) if self.res else np.zeros(0, dtype=pkg.WANTED_RES)
        return dict(opt=sam_opt(self.flag), pes=pes_fr() if self.flag & PE else None, seqs=self.seqs, vectors=self.vectors, dec=dec, res=res,
                    cig=np.array(self.cig + [0], dtype=np.uint32), md=np.frombuffer(bytes(self.md) + b"\0", dtype=np.uint8).copy(), rg_id=rg_id)


def _se_read(b, u):
    """single-end read number u: the shapes by its number"""
    rng = b.rng
    kind = u % 16
    s = b.read(l_seq=1 if kind == 5 else None, qual=kind != 3, comment=kind in (2, 6, 7), name=(b"n", b"N" * 250)[u % 32 // 16] if kind == 4 else None)
    n = len(s[2])
    if kind == 5:  # one base, unmapped
        return b.add(s, [])
    if kind == 6:  # no wanted region, with and without a vector
        return b.add(s, [], n_junk=u % 32 // 16)
    where = (1, EDGES[(u // 16) % len(EDGES)]) if kind == 0 else (3, int(rng.integers(2_000_000_000, 2_146_990_000))) if kind == 1 else None
    first = b.region(n, where=where, rev=bool(u // 16 % 2) if kind in (0, 1) else None, kind=("plain", "lead", "trail")[u % 3],
                     clip=("none", "5", "3", "both")[u // 3 % 4])
    regs = [first]
    if kind == 7:  # >= 40 printed regions: supplementary and, with ALL, secondary lines
        for k in range(44):
            regs.append(b.region(n, secondary=0 if (b.flag & ALL and k % 3 == 0) else -1))
    elif kind in (8, 9):  # one supplementary line: SA:Z with one other line
        regs.append(b.region(n, clip=("5", "3", "both")[u % 3], rev=bool(u % 2)))
    elif kind in (10, 11):  # SA:Z with >= 3 other lines
        regs += [b.region(n) for _ in range(3 + u % 3)]
    elif kind == 12 and b.flag & ALL:  # secondary lines only
        regs += [b.region(n, secondary=0) for _ in range(2)]
    b.add(s, regs, n_junk=u % 2)


def _pair(b, p):
    """pair number p: the shapes by its number"""
    rng, pkg = b.rng, load_package()
    kind = p % 12
    name = b"pair%d" % p
    s = [b.read(name=name, qual=kind != 3, comment=kind == 2), b.read(name=name, l_seq=1 if kind == 5 else None, qual=kind != 3, comment=kind == 2)]
    d = np.zeros((), dtype=pkg.PAIRDEC)
    d["extra_flag"] = 1
    ci = (0, 1, 3)[p // 12 % 3]
    room = CONTIGS[ci][1]
    if kind in (0, 1, 2, 3, 4):  # a paired decision; TLEN d > 0, d < 0, d == 0 and distances of 1 to 10 digits in the long sequences
        gap = p // 12 % 4 * 3 if kind == 4 else 10 ** (p // 12 % 10) if ci else int(rng.integers(0, 900))  # (kind 4: TLEN 0, 4, 7, 10 either way)
        p0 = int(rng.integers(0, max(room - gap - 1000, 1)))
        order = p // 24 % 2 if kind == 4 else p % 2
        ends = [b.region(len(s[0][2]), where=(ci, p0 + (gap if order else 0)), rev=kind != 4 and bool(order), kind="plain" if kind != 1 else "lead"),
                b.region(len(s[1][2]), where=(ci, p0 + (0 if order else gap)), rev=kind != 4 and not order)]  # (kind 4: both forward)
        d["paired"], d["extra_flag"], d["q_se"] = 1, 3, (int(rng.integers(0, 61)), int(rng.integers(0, 61)))
        d["z"] = (p % 3 == 0, 0)  # z[] need not be the first region
        for r in range(2):
            _add_paired(b, s[r], [] if d["z"][r] == 0 else [b.region(len(s[r][2]), score=T + 200, pool=False)[0]], ends[r])
        b.pd.append(d)
        return
    if kind == 5:  # a paired decision whose second end has nothing to print: its place is borrowed, bit 0x8 on the other line
        e0 = b.region(len(s[0][2]), where=(ci, int(rng.integers(0, room - 400))))
        d["paired"], d["extra_flag"], d["q_se"] = 1, 3, (17, 0)
        b.add(s[0], [e0])
        b.add(s[1], [])
        b.pd.append(d)
        return
    # unpaired ends through mem_reg2sam_se with the other end's top hit as mate
    if kind == 6:  # one end without a hit
        b.add(s[0], [b.region(len(s[0][2])), b.region(len(s[0][2]))])
        b.add(s[1], [], n_junk=p // 12 % 2)
    elif kind == 7:  # the mates in different sequences
        b.add(s[0], [b.region(len(s[0][2]), where=(0, int(rng.integers(0, 4000))))])
        b.add(s[1], [b.region(len(s[1][2]), where=(3, int(rng.integers(0, 1 << 31))))])
    elif kind == 11:  # neither end has a hit
        b.add(s[0], [])
        b.add(s[1], [])
    else:  # both ends in chr1, FR: inside the model's bounds (a proper pair) or outside them
        far = kind in (9, 10)
        p0 = int(rng.integers(0, 1000))
        e0 = [b.region(len(s[0][2]), where=(0, p0), rev=False, clip="none")]
        e1 = [b.region(len(s[1][2]), where=(0, p0 + (3000 if far else 300)), rev=True, clip="none")]
        if kind in (8, 10):
            e0.append(b.region(len(s[0][2]), clip="5"))
            e1 += [b.region(len(s[1][2]), secondary=0)] if b.flag & ALL else []
        b.add(s[0], e0, n_junk=1)
        b.add(s[1], e1)
    b.pd.append(d)


def _add_paired(b, s, before, end):
    """an end of a paired decision: the chosen region alone is wanted, possibly behind a region that is not"""
    vec = list(before) + [end[0]]
    b.res.append(end[1])
    b.seqs.append(s), b.want.append(np.array([len(before)], dtype=np.int32))
    b.vectors.append(np.array(vec, dtype=kswlib.ALNREG).reshape(-1))
    b.mapq.append(b.rng.integers(0, 61, len(vec)).astype(np.int32))


def make(mode, units, seed=0, rg_id=None, flag=0):
    """A slice of `units` reads or pairs.  mode: "se", "se-all", "pe", "pe-all"; flag: more mem_opt_t.flag bits (NO_MULTI, NOPAIRING)."""
    pe = mode.startswith("pe")
    flag |= (PE if pe else 0) | (ALL if mode.endswith("all") else 0)
    rng = np.random.default_rng([seed, units, flag])
    b = Builder(rng, flag)
    for u in range(units):
        (_pair if pe else _se_read)(b, u)
    return b.done(rg_id if rg_id is not None else (b"", b"grp1.lane-3")[seed % 2])


def expected(sl):
    """the restatement's text of a slice: per read its lines"""
    import samtext_ref as ref
    return ref.slice_text(sl["opt"], CONTIGS, NAMES, L_PAC, sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"], sl["cig"], sl["md"], sl["rg_id"])


def shapes(sl, texts):
    """what a slice's text contains, counted from the lines themselves"""
    s = dict(lines=0, secondary=0, supplementary=0, hard=0, sa1=0, sa3=0, unmapped=0, many=0, mate_unmapped=0, mate_other=0, tlen_pos=0, tlen_neg=0,
             tlen_zero=0, proper=0, improper=0, no_qual=0, comment=0, rg=0, neg_tlen_digits=set(), pos_digits=set(), rev_past_2_32=0,
             lead_trail_del=0, name_lens=set(), l_seq_1=0, no_multi=0, capped=0, top_proper=0, top_improper=0)
    pe = bool(int(sl["opt"]["flag"]) & PE)
    roff = np.concatenate([[0], np.cumsum([len(v) for v in sl["vectors"]])])
    for i, ((name, com, seq, qual), v, ks, t) in enumerate(zip(sl["seqs"], sl["vectors"], sl["dec"]["want"], texts)):
        lines = t.split(b"\n")[:-1]
        unpaired = pe and not int(sl["dec"]["pd"][i // 2]["paired"])
        s["top_proper"] += unpaired and bool(int(lines[0].split(b"\t")[1]) & 0x2)
        s["top_improper"] += unpaired and not int(lines[0].split(b"\t")[1]) & 0x2
        mq = sl["dec"]["reg_mapq"][int(roff[i]):]
        s["capped"] += (not pe or unpaired) and any(int(v[int(k)]["secondary"]) < 0 and mq[int(k)] > mq[int(ks[0])] for k in ks[1:])
        s["lines"] += len(lines)
        s["many"] += len(lines) >= 40
        s["name_lens"].add(len(name))
        s["l_seq_1"] += len(seq) == 1
        for ln in lines:
            f = ln.split(b"\t")
            flag, tlen = int(f[1]), int(f[8])
            s["secondary"] += bool(flag & 0x100) and f[9] == b"*"
            s["supplementary"] += bool(flag & 0x800)
            s["no_multi"] += bool(flag & 0x100) and f[9] != b"*"
            s["hard"] += b"H" in f[5]
            sa = [x for x in f[11:] if x.startswith(b"SA:Z:")]
            s["sa1"] += bool(sa) and sa[0].count(b";") == 1
            s["sa3"] += bool(sa) and sa[0].count(b";") >= 3
            s["unmapped"] += bool(flag & 0x4)
            s["mate_unmapped"] += bool(flag & 0x8) and not flag & 0x4 and f[6] == b"="
            s["mate_other"] += f[6] not in (b"=", b"*")
            s["tlen_pos"] += tlen > 0
            s["tlen_neg"] += tlen < 0
            s["tlen_zero"] += tlen == 0 and f[6] == b"=" and f[5] != b"*" and not flag & 0x8
            s["proper"] += bool(flag & 0x2)
            s["improper"] += bool(flag & 0x1) and not flag & 0x2
            s["no_qual"] += f[10] == b"*" and f[9] != b"*"
            s["comment"] += com is not None
            s["rg"] += any(x.startswith(b"RG:Z:") for x in f[11:])
            s["pos_digits"].add(len(f[3]))
            if tlen < 0:
                s["neg_tlen_digits"].add(len(f[8]) - 1)
        for k in ks:
            a = v[int(k)]
            s["rev_past_2_32"] += int(a["rb"]) > 1 << 32
    for x in sl["res"]:
        w = sl["cig"][int(x["cigar_off"]):int(x["cigar_off"]) + int(x["n_cigar"])]
        s["lead_trail_del"] += len(w) > 0 and (int(w[0]) & 0xf == 2 or int(w[-1]) & 0xf == 2)
    return s


def sentinels(n):
    return {"text": C.c_void_p(0x5a5a5a5a), "text_off": np.full(n + 1, -77, dtype=np.int64)}


def refusals(sl):
    """(what, a broken copy of the slice's arguments) for everything both forms refuse"""
    def cp(**kw):
        d = dict(sl)
        d["dec"] = dict(sl["dec"])
        for k, v in kw.items():
            if k in d["dec"]:
                d["dec"][k] = v
            else:
                d[k] = v
        return d
    n = len(sl["seqs"])
    nw = sl["dec"]["n_want"].copy()
    nw[0] = -1
    big = sl["dec"]["n_want"].copy()
    big[0] = len(sl["vectors"][0]) + 1
    first_wanted = int(np.flatnonzero(sl["dec"]["n_want"])[0])
    roff0 = int(sum(len(v) for v in sl["vectors"][:first_wanted]))
    wk = sl["dec"]["want_k"].copy()
    wk[roff0] = len(sl["vectors"][first_wanted])
    res_q = sl["res"].copy()
    res_q["qe"][0] = 100000
    res_c = sl["res"].copy()
    res_c["n_cigar"][0] = -1
    res_r = sl["res"].copy()
    res_r["rb"][0], res_r["re"][0] = L_PAC - 5, L_PAC - 1  # fine ...
    res_r["rb"][0] = -9  # ... but before the reference
    noname = list(sl["seqs"])
    noname[0] = (None,) + tuple(noname[0][1:])
    out = [("n_want < 0", cp(n_want=nw)), ("n_want past the vector", cp(n_want=big)), ("want_k past the vector", cp(want_k=wk)),
           ("no records", cp(res=None)), ("no CIGAR pool", cp(cig=None)), ("no MD pool", cp(md=None)), ("no reg_mapq", cp(reg_mapq=None)),
           ("no n_want", cp(n_want=None)), ("no want_k", cp(want_k=None)), ("a record past its read", cp(res=res_q)),
           ("a negative CIGAR count", cp(res=res_c)), ("a record before the reference", cp(res=res_r)), ("a read without a name", cp(seqs=noname))]
    if int(sl["opt"]["flag"]) & PE:
        names = list(sl["seqs"])
        names[1] = (b"other",) + tuple(names[1][1:])
        out += [("mates with different names", cp(seqs=names)), ("no pes", cp(pes=None)),
                ("an odd number of reads", cp(seqs=sl["seqs"][:-1], vectors=sl["vectors"][:-1]))]
    return out


def pack_reads(seqs):
    """the read pool as bmh_sam_text_device uploads it: per read 16 bytes of lengths, name, codes, qualities, comment, rounded up to 8"""
    poff, pool = [0], bytearray()
    for name, com, seq, qual in seqs:
        b = np.array([len(name), len(seq), qual is not None, len(com) if com is not None else -1], dtype=np.int32).tobytes()
        b += name + bytes(np.asarray(seq, dtype=np.uint8).tolist()) + (qual or b"") + (com or b"")
        pool += b + b"\0" * (-len(b) % 8)
        poff.append(len(pool))
    return np.array(poff, dtype=np.uint64), bytes(pool)
