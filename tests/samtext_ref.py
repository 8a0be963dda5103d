"""Pass C of phase 2 restated in Python from the reference's own lines: mem_reg2aln's second half (bwa-0.7.8/bwamem.c:1203-1235),
mem_aln2sam (:904-1017), mem_reg2sam_se (:1049-1083) and the two tails of mem_sam_pe (bwamem_pair.c:306-331).  Independent of
host/samtext_core.h: it works on Python lists and byte strings, keeps a clipped copy of every CIGAR as the reference does, and prints
numbers with Python's own formatting.  The tests compare bmh_sam_text_batch and bmh_sam_text_device with it byte for byte."""

NOPAIRING, NO_MULTI, PE = 0x4, 0x10, 0x2


class Aln:  # mem_aln_t, bwamem.h:72-82; cigar a list of words, md the MD string
    def __init__(self):
        self.pos, self.rid, self.flag, self.is_rev, self.mapq, self.NM, self.score, self.sub = -1, -1, 0x4, 0, 0, 0, 0, 0
        self.cigar, self.md = [], b""

    def copy(self):
        c = Aln()
        c.__dict__.update(self.__dict__)
        c.cigar = list(self.cigar)
        return c


def pos2rid(contigs, l_pac, pos):  # bns_pos2rid, bntseq.c:316-330
    if pos >= l_pac:
        return -1
    rid = 0
    for i, c in enumerate(contigs):
        if pos >= c[0]:
            rid = i
    return rid


def reg2aln(contigs, l_pac, l_query, reg, x, mapq, cig, md):
    """bwamem.c:1171-1235 given the alignment (x: the wanted region's record, its CIGAR and MD in the pools); reg None: unmapped"""
    a = Aln()
    if reg is None:
        return a
    a.flag = 0
    a.mapq = mapq if int(reg["secondary"]) < 0 else 0
    if int(reg["secondary"]) >= 0:
        a.flag |= 0x100
    qb, qe, rb, re = int(x["qb"]), int(x["qe"]), int(x["rb"]), int(x["re"])
    words = [int(w) for w in cig[int(x["cigar_off"]):int(x["cigar_off"]) + int(x["n_cigar"])]]
    a.md = bytes(md[int(x["md_off"]):int(x["md_off"]) + int(x["md_len"])])
    a.NM = int(x["NM"])
    pos = rb if rb < l_pac else re - 1
    a.is_rev = int(pos >= l_pac)  # bns_depos
    if a.is_rev:
        pos = (l_pac << 1) - 1 - pos
    if words:  # squeeze out leading or trailing deletions
        if words[0] & 0xf == 2:
            pos += words[0] >> 4
            words = words[1:]
        elif words[-1] & 0xf == 2:
            words = words[:-1]
    if qb != 0 or qe != l_query:  # add clipping to CIGAR
        clip5 = l_query - qe if a.is_rev else qb
        clip3 = qb if a.is_rev else l_query - qe
        if clip5:
            words = [clip5 << 4 | 3] + words
        if clip3:
            words = words + [clip3 << 4 | 3]
    a.cigar = words
    a.rid = pos2rid(contigs, l_pac, pos)
    a.pos = pos - contigs[a.rid][0]
    a.score = int(reg["score"])
    a.sub = max(int(reg["sub"]), int(reg["csub"]))
    return a


def _rlen(cigar):  # get_rlen
    return sum(w >> 4 for w in cigar if w & 0xf in (0, 2))


def aln2sam(names, rg_id, s, lst, which, m_):
    """mem_aln2sam, bwamem.c:904-1017.  s: (name, comment or None, base codes, qualities or None)"""
    name, comment, seq, qual = s
    p = lst[which].copy()
    m = m_.copy() if m_ is not None else None
    p.flag |= 0x1 if m else 0
    p.flag |= 0x4 if p.rid < 0 else 0
    p.flag |= 0x8 if m and m.rid < 0 else 0
    if p.rid < 0 and m and m.rid >= 0:  # copy mate to alignment
        p.rid, p.pos, p.is_rev, p.cigar = m.rid, m.pos, m.is_rev, []
    if m and m.rid < 0 and p.rid >= 0:  # copy alignment to mate
        m.rid, m.pos, m.is_rev, m.cigar = p.rid, p.pos, p.is_rev, []
    p.flag |= 0x10 if p.is_rev else 0
    p.flag |= 0x20 if m and m.is_rev else 0
    out = [name, b"\t", b"%d" % ((p.flag & 0xffff) | (0x100 if p.flag & 0x10000 else 0)), b"\t"]
    if p.rid >= 0:
        out += [names[p.rid], b"\t", b"%d" % (p.pos + 1), b"\t", b"%d" % p.mapq, b"\t"]
        if p.cigar:
            for w in p.cigar:
                c = w & 0xf
                if c in (3, 4):
                    c = 4 if which else 3
                out.append(b"%d%c" % (w >> 4, b"MIDSH"[c]))
        else:
            out.append(b"*")
    else:
        out.append(b"*\t0\t0\t*")
    out.append(b"\t")
    if m and m.rid >= 0:
        out += [b"=" if p.rid == m.rid else names[m.rid], b"\t", b"%d" % (m.pos + 1), b"\t"]
        if p.rid == m.rid:
            p0 = p.pos + (_rlen(p.cigar) - 1 if p.is_rev else 0)
            p1 = m.pos + (_rlen(m.cigar) - 1 if m.is_rev else 0)
            if not m.cigar or not p.cigar:
                out.append(b"0")
            else:
                out.append(b"%d" % -(p0 - p1 + (1 if p0 > p1 else -1 if p0 < p1 else 0)))
        else:
            out.append(b"0")
    else:
        out.append(b"*\t0\t0")
    out.append(b"\t")
    if p.flag & 0x100:
        out.append(b"*\t*")
    else:
        qb, qe = 0, len(seq)
        if p.cigar:
            first, last = p.cigar[0], p.cigar[-1]
            if which and first & 0xf in (3, 4):
                if p.is_rev:
                    qe -= first >> 4
                else:
                    qb += first >> 4
            if which and last & 0xf in (3, 4):
                if p.is_rev:
                    qb += last >> 4
                else:
                    qe -= last >> 4
        idx = range(qe - 1, qb - 1, -1) if p.is_rev else range(qb, qe)
        out.append(bytes((b"TGCAN" if p.is_rev else b"ACGTN")[int(seq[i])] for i in idx))
        out.append(b"\t")
        out.append(bytes(qual[i] for i in idx) if qual is not None else b"*")
    if p.cigar:
        out += [b"\tNM:i:%d" % p.NM, b"\tMD:Z:", p.md]
    if p.score >= 0:
        out.append(b"\tAS:i:%d" % p.score)
    if p.sub >= 0:
        out.append(b"\tXS:i:%d" % p.sub)
    if rg_id:
        out += [b"\tRG:Z:", rg_id]
    if not p.flag & 0x100:
        others = [r for i, r in enumerate(lst) if i != which and not r.flag & 0x100]
        if others:
            out.append(b"\tSA:Z:")
            for r in others:
                out += [names[r.rid], b",%d,%c," % (r.pos + 1, b"+-"[r.is_rev]), b"".join(b"%d%c" % (w >> 4, b"MIDSH"[w & 0xf]) for w in r.cigar),
                        b",%d,%d;" % (r.mapq, r.NM)]
    if comment is not None:
        out += [b"\t", comment]
    out.append(b"\n")
    return b"".join(out)


def reg2sam_se(opt_flag, names, rg_id, s, ks, regs, alns, extra_flag, m):
    """mem_reg2sam_se, bwamem.c:1049-1083, over the regions pass A selected (ks, in its order) and their mem_reg2aln results"""
    aa = []
    for k, q in zip(ks, alns):
        p = regs[k]
        q.flag |= extra_flag
        if int(p["secondary"]) >= 0:
            q.sub = -1
        if k and int(p["secondary"]) < 0:
            q.flag |= 0x10000 if opt_flag & NO_MULTI else 0x800
        aa.append(q)
        if k and q.mapq > aa[0].mapq:
            q.mapq = aa[0].mapq
    if not aa:
        t = Aln()
        t.flag |= extra_flag
        return aln2sam(names, rg_id, s, [t], 0, m)
    return b"".join(aln2sam(names, rg_id, s, aa, k, m) for k in range(len(aa)))


def infer_dir(l_pac, b1, b2):  # mem_infer_dir, bwamem_pair.c:25-32
    r1, r2 = int(b1 >= l_pac), int(b2 >= l_pac)
    p2 = b2 if r1 == r2 else (l_pac << 1) - 1 - b2
    dist = p2 - b1 if p2 > b1 else b1 - p2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), dist


def slice_text(opt, contigs, names, l_pac, pes, seqs, vectors, dec, res, cig, md, rg_id=b""):
    """every read's SAM lines: worker2 (bwamem.c:1281-1295) after the decisions.  dec: pd, reg_mapq, want (per read the printed regions)"""
    flag, T = int(opt["flag"]), int(opt["T"])
    roff = [0]
    for v in vectors:
        roff.append(roff[-1] + len(v))
    alns, j = [], 0
    for i, ks in enumerate(dec["want"]):  # mem_reg2aln of every wanted region, in want order
        mine = []
        for k in ks:
            mine.append(reg2aln(contigs, l_pac, len(seqs[i][2]), vectors[i][int(k)], res[j], int(dec["reg_mapq"][roff[i] + int(k)]), cig, md))
            j += 1
        alns.append(mine)
    out = []
    if not flag & PE:
        for i in range(len(seqs)):
            out.append(reg2sam_se(flag, names, rg_id, seqs[i], [int(k) for k in dec["want"][i]], vectors[i], alns[i], 0, None))
        return out
    for p in range(len(seqs) // 2):
        d, i = dec["pd"][p], 2 * p
        extra = int(d["extra_flag"])
        if int(d["paired"]):  # bwamem_pair.c:311-315
            h = []
            for r in range(2):
                a = alns[i + r][0].copy() if alns[i + r] else Aln()
                a.mapq = int(d["q_se"][r])
                a.flag |= (0x80 if r else 0x40) | extra
                h.append(a)
            out += [aln2sam(names, rg_id, seqs[i], [h[0]], 0, h[1]), aln2sam(names, rg_id, seqs[i + 1], [h[1]], 0, h[0])]
            continue
        h = []
        for r in range(2):  # no_pairing, :320-331
            v = vectors[i + r]
            top = len(v) and int(v[0]["score"]) >= T and len(dec["want"][i + r]) and int(dec["want"][i + r][0]) == 0
            h.append(alns[i + r][0].copy() if top else Aln())
        if not flag & NOPAIRING and h[0].rid == h[1].rid and h[0].rid >= 0:
            dd, dist = infer_dir(l_pac, int(vectors[i][0]["rb"]), int(vectors[i + 1][0]["rb"]))
            if not int(pes[dd]["failed"]) and int(pes[dd]["low"]) <= dist <= int(pes[dd]["high"]):
                extra |= 2
        for r in range(2):
            out.append(reg2sam_se(flag, names, rg_id, seqs[i + r], [int(k) for k in dec["want"][i + r]], vectors[i + r], alns[i + r],
                                  (0x81 if r else 0x41) | extra, h[1 - r]))
    return out
