"""Generator and reference of the region-record tests whose CIGAR or MD outgrow the fixed slots (bmh_region_cigar_batch_long):
regions on a 60 kb reference with planted indels and substitutions, as requests of bmh_reg2cigar_batch (CIGAR_REQ) and -- through a
restatement of host/regplan_core.h's plan, which tests/regfinish_core_main.c checks against the header -- as the records and tasks
bmh_region_cigar_batch takes.  The reference of a region is the oracle's ksw_global2 on oriented copies made in numpy, the band loop
(reference bwa-0.7.8/bwamem.c:1194-1201) replayed here and a restatement of bwa.c:134-164; it is computed once per region and cached.

Classes, from the oracle alone (CIG_CAP words, MD_CAP bytes): CIGAR-cut, MD-cut (the CIGAR fits), both, each strand, the index of the
final try.  CLASS_MIN of each must be there; the two 12 000-base regions (one per strand, w = 100, a single try) are the ring kernel's."""
import functools

import numpy as np

import kswlib

L_PAC = 60000
CIG_CAP, MD_CAP = 24, 96
CLASS_MIN = 8
INT_MIN = -2 ** 31
REGION_REQ = np.dtype([("q_src", "<u8"), ("rb", "<i8"), ("o_off", "<u8"), ("ql", "<i4"), ("tl", "<i4"), ("truesc", "<i4"),
                       ("task", "<i4", (3,))])


@functools.lru_cache(maxsize=None)
def genome():
    """(bases, pac, doubled coordinate as one code per byte)"""
    rng = np.random.default_rng(20260)
    bases = rng.integers(0, 4, L_PAC, dtype=np.uint8)
    q4 = np.concatenate([bases, np.zeros((-L_PAC) % 4 + 4, np.uint8)])
    q4 = q4[: (len(q4) // 4) * 4].reshape(-1, 4)
    pac = (q4[:, 0] << 6 | q4[:, 1] << 4 | q4[:, 2] << 2 | q4[:, 3]).astype(np.uint8)
    return bases, pac, np.concatenate([bases, (3 - bases)[::-1]])


# ---- host/regplan_core.h, restated (bwamem.c:884-891, :1187-1191, bwa.c:116-125)
def _infer_bw(l1, l2, score, a, q, r):
    if l1 == l2 and l1 * a - score < (q + r - a) * 2:
        return 0
    w = int((min(l1, l2) * a - score - q) / r + 2.)
    return max(w, abs(l1 - l2))


def first_band(p, ql, tl, truesc, reg_w):
    if truesc == INT_MIN:
        return reg_w
    a = int(p["a"])
    w2 = max(_infer_bw(ql, tl, truesc, a, int(p["o_del"]), int(p["e_del"])), _infer_bw(ql, tl, truesc, a, int(p["o_ins"]), int(p["e_ins"])))
    return min(w2, reg_w) if w2 > int(p["w"]) else w2


def try_band(p, ql, tl, w2):
    m0 = int(p["mat"][0])
    max_ins = int((((ql + 1) >> 1) * m0 - int(p["o_ins"])) / int(p["e_ins"]) + 1.)
    max_del = int((((ql + 1) >> 1) * m0 - int(p["o_del"])) / int(p["e_del"]) + 1.)
    w = (max(max_ins, max_del, 1) + abs(tl - ql) + 1) >> 1
    return max(min(w, w2), abs(tl - ql) + 3)


def plan(p, ql, tl, truesc, reg_w):
    """(band of each try or -1, task slot of each try or -1, tasks); no task at all: the no-gap case"""
    single = truesc == INT_MIN
    w2 = first_band(p, ql, tl, truesc, reg_w)
    band, slot, n, prev = [-1] * 3, [-1] * 3, 0, -1
    if ql == tl and w2 == 0:
        return band, slot, 0
    for t in range(1 if single else 3):
        w = try_band(p, ql, tl, min(w2 << t, 2 ** 31 - 1) if w2 >= 0 else w2)
        band[t] = w
        if w == prev:
            slot[t] = slot[t - 1]
            continue
        prev = w
        slot[t] = n
        n += 1
    return band, slot, n


# ---- the regions
def _planted(rng, src, n_indel, sub, size=(1, 4), gap=30, balanced=True):
    """A read made from src: n_indel indels at least `gap` matching bases apart -- alternately deleted from the read and inserted, so
    that the lengths stay close -- and substitutions at rate `sub`.  Returns (read, reference bases used)."""
    out, i = [], 0
    room = len(src) - 8 * n_indel - 2 * gap
    cuts = np.sort(rng.choice(np.arange(gap, max(room, gap + n_indel * gap), gap), size=n_indel, replace=False)) if n_indel else []
    for k, c in enumerate(cuts):
        out.append(src[i:c])
        d = int(rng.integers(size[0], size[1]))
        if (k & 1) if balanced else rng.random() < 0.5:
            ins = rng.integers(0, 4, d).astype(np.uint8)
            ins[0] = (src[c] + 1) & 3  # (never the base that follows: the insertion cannot slide away)
            out.append(ins)
            i = c
        else:
            i = c + d
    out.append(src[i:])
    read = np.concatenate(out).astype(np.uint8)
    mut = rng.random(len(read)) < sub
    read[mut] = (read[mut] + rng.integers(1, 4, int(mut.sum()))) & 3
    return read


def _region(rng, kind, k, L, **kw):
    """One region of the forward strand's bases [pos, pos + span), on the strand k & 1.  -> dict(read, rb, re, truesc, reg_w, kind)"""
    bases, _, dbl = genome()
    rev = k & 1
    pos = int(rng.integers(50, L_PAC - L - 400))
    lead, trail = kw.get("lead", 0), kw.get("trail", 0)  # window bases before / behind what the read covers: a deletion as the first / last operation
    src = bases[pos:pos + L]
    read = _planted(rng, src, kw.get("n_indel", 0), kw.get("sub", 0.), kw.get("size", (1, 4)), kw.get("gap", 30))
    if kw.get("n_base"):
        read[rng.integers(0, len(read), kw["n_base"])] = 4
    rb, re = pos - lead, pos + L + trail
    if rev:  # the read is the reverse complement (N stays N), the region lies in [l_pac, 2 * l_pac)
        read = np.where(read < 4, 3 - read, 4).astype(np.uint8)[::-1].copy()
        rb, re = 2 * L_PAC - re, 2 * L_PAC - rb
    ql = len(read)
    truesc = kw["truesc"](ql) if callable(kw.get("truesc")) else kw.get("truesc", ql - 60)
    return dict(read=read, rb=rb, re=re, truesc=int(truesc), reg_w=int(kw.get("reg_w", 100)), kind=kind)


@functools.lru_cache(maxsize=None)
def regions():
    """The generator's regions: (flagged kinds..., "short" ones that fit their slots)."""
    rng = np.random.default_rng(4711)
    out = []
    k = 0

    def add(kind, n, L, **kw):
        nonlocal k
        for _ in range(n):
            LL = int(rng.integers(L[0], L[1])) if isinstance(L, tuple) else L
            out.append(_region(rng, kind, k, LL, **kw))
            k += 1
    # CIGARs of 25 and 64 operations (12 indels: 2n + 1 operations; 31 and a deletion in front), 26 with a deletion in front, about 300; ql 200 .. 2 000
    add("cig25", 4, (420, 520), n_indel=12, truesc=lambda ql: ql - 80)
    add("cig26", 4, (420, 520), n_indel=12, lead=2, truesc=INT_MIN, reg_w=40)
    add("cig64", 4, (1100, 1300), n_indel=31, lead=2, truesc=lambda ql: ql - 200)
    add("cig300", 4, (1900, 2000), n_indel=150, gap=12, size=(1, 3), truesc=INT_MIN, reg_w=100)
    add("cig_n", 4, (500, 700), n_indel=16, n_base=3, truesc=lambda ql: ql - 100)
    # a deletion as the first and as the last operation
    add("del_first", 4, (450, 600), n_indel=13, lead=3, truesc=INT_MIN, reg_w=30)
    add("del_last", 4, (450, 600), n_indel=13, trail=3, truesc=INT_MIN, reg_w=30)
    # MD past MD_CAP with the CIGAR within CIG_CAP: 300 bases, 30 % substitutions; with a band (one try) and as the no-gap case
    add("md_only", 10, 300, sub=0.3, truesc=INT_MIN, reg_w=5)
    add("md_nogap", 6, 300, sub=0.3, truesc=lambda ql: ql - 5)
    add("md_indel", 6, (280, 320), n_indel=3, sub=0.25, truesc=lambda ql: ql - 250)
    # both too long
    add("both", 10, (700, 900), n_indel=20, sub=0.06, truesc=lambda ql: ql - 400)
    # narrow first bands: the final try is the 2nd (the score repeats) or the 3rd (the 1st band cuts a gap pair the 2nd holds)
    add("try2", 10, (500, 600), n_indel=14, truesc=lambda ql: ql)
    add("try3", 18, (500, 600), n_indel=14, size=(6, 8), truesc=lambda ql: ql - 8)
    add("try3b", 6, (500, 600), n_indel=14, size=(10, 14), truesc=lambda ql: ql - 8)
    # the ring kernel's: 12 000 bases, one per strand, w = 100
    add("ring", 2, 12000, n_indel=120, gap=60, sub=0.01, truesc=INT_MIN, reg_w=100)
    # ordinary ones, which fit their slots
    add("short", 40, (60, 160), sub=0.03, truesc=lambda ql: ql - 20)
    add("short_indel", 30, (80, 160), n_indel=1, sub=0.02, truesc=lambda ql: ql - 30)
    add("short_one", 10, (60, 160), n_indel=1, truesc=INT_MIN, reg_w=20)
    return tuple(out)


def oriented(r):
    """the oriented copies of bwa.c:100-107: (query, window, rev)"""
    _, _, dbl = genome()
    rev = r["rb"] >= L_PAC
    q, t = r["read"], dbl[r["rb"]:r["re"]]
    return (q[::-1].copy(), t[::-1].copy(), True) if rev else (q.copy(), t.copy(), False)


def md_of(words, q, t, rev):
    """bwa.c:134-164 on oriented copies -> (NM, MD bytes)"""
    b2c = b"TGCAN" if rev else b"ACGTN"
    x = y = u = mm = gap = 0
    out = bytearray()
    for k, wd in enumerate(words):
        op, ln = int(wd) & 0xf, int(wd) >> 4
        if op == 0:
            neq = np.nonzero(q[x:x + ln] != t[y:y + ln])[0]
            last = -1
            for i in neq:
                u += int(i) - last - 1
                out += str(u).encode() + b2c[t[y + i]:t[y + i] + 1]
                mm, u, last = mm + 1, 0, int(i)
            u += ln - last - 1
            x, y = x + ln, y + ln
        elif op == 2:
            if 0 < k < len(words) - 1:
                out += str(u).encode() + b"^" + bytes(b2c[c] for c in t[y:y + ln])
                u, gap = 0, gap + ln
            y += ln
        elif op == 1:
            x, gap = x + ln, gap + ln
    out += str(u).encode()
    return mm + gap, bytes(out)


_REF = {}


def reference(p, idx):
    """dict(score, words, tries, fin (try index the loop ends on, -1: the no-gap case), NM, md) of regions()[idx] under the default
    scoring p; cached."""
    if idx in _REF:
        return _REF[idx]
    r = regions()[idx]
    q, t, rev = oriented(r)
    ql, tl = len(q), len(t)
    band, slot, n = plan(p, ql, tl, r["truesc"], r["reg_w"])
    a = int(p["a"])
    single = r["truesc"] == INT_MIN
    if n == 0:
        mat = np.array(p["mat"], dtype=np.int64).reshape(5, 5)
        sc = int(mat[t, q].sum())
        words, tries, fin = np.array([ql << 4], dtype=np.uint32), (2 if (not single and sc < r["truesc"] - a) else 1), -1
    else:
        pool = np.concatenate([q, t, np.zeros(16, np.uint8)])
        tasks = np.zeros(n, dtype=kswlib.GLB_TASK)
        for t_ in range(3):
            if slot[t_] >= 0:
                tasks[slot[t_]] = (0, ql, ql, tl, band[t_], 0, 1)
        ores, ocig = kswlib.orc_global_batch(p, pool, tasks)
        last, tries = -(1 << 30), 0
        for t_ in range(3):
            fin = t_
            tries += 1
            sc = int(ores[slot[t_]]["score"])
            if sc == last:
                break
            last = sc
            if single or not (tries < 3 and sc < r["truesc"] - a):
                break
        words = ocig[slot[fin]]
    nm, md = md_of(words, q, t, rev)
    _REF[idx] = dict(score=sc, words=words, tries=tries, fin=fin, NM=nm, md=md)
    return _REF[idx]


def classes(p, cig_cap=CIG_CAP, md_cap=MD_CAP):
    """From the oracle alone: how many regions fall into each class the long round must handle."""
    c = dict(cigar_cut=0, md_cut=0, both=0, fwd=0, rev=0, fin0=0, fin1=0, fin2=0, ring_fwd=0, ring_rev=0, del_first=0, del_last=0,
             n_base=0, one_try=0, nogap_md=0, unflagged=0, n25=0, n26=0, n64=0, n300=0)
    for i, r in enumerate(regions()):
        x = reference(p, i)
        n, m = len(x["words"]), len(x["md"])
        if n <= cig_cap and m <= md_cap:
            c["unflagged"] += 1
            continue
        rev = r["rb"] >= L_PAC
        c["cigar_cut"] += n > cig_cap
        c["md_cut"] += n <= cig_cap and m > md_cap
        c["both"] += n > cig_cap and m > md_cap
        c["rev" if rev else "fwd"] += 1
        if x["fin"] >= 0:
            c["fin%d" % x["fin"]] += 1
        else:
            c["nogap_md"] += 1
        if len(r["read"]) >= 12000 - 400:
            c["ring_rev" if rev else "ring_fwd"] += 1
        c["del_first"] += int(x["words"][0]) & 0xf == 2
        c["del_last"] += int(x["words"][-1]) & 0xf == 2
        c["n_base"] += bool((r["read"] == 4).any())
        c["one_try"] += r["truesc"] == INT_MIN
        c["n25"] += n == 25
        c["n26"] += n == 26
        c["n64"] += n == 64
        c["n300"] += 260 <= n <= 340
    return c


def check_classes(c):
    for k in ("cigar_cut", "md_cut", "both", "fwd", "rev", "fin0", "fin1", "fin2"):
        assert c[k] >= CLASS_MIN, (k, c)
    assert c["ring_fwd"] >= 1 and c["ring_rev"] >= 1, c
    for k in ("del_first", "del_last", "n_base", "one_try", "nogap_md", "n25", "n26", "n64", "n300"):
        assert c[k] >= 1, (k, c)
    assert c["unflagged"] >= 40, c


# ---- the two request forms
def cigar_reqs(idxs):
    """(reads, CIGAR_REQ array) of bmh_reg2cigar_batch / orc_reg2cigar for the regions idxs, whole reads as the query"""
    rs = regions()
    reads, reqs = [], np.zeros(len(idxs), dtype=kswlib.CIGAR_REQ)
    for j, i in enumerate(idxs):
        r = rs[i]
        reads.append(r["read"])
        reqs[j] = (j, 0, len(r["read"]), 0, r["rb"], r["re"], r["truesc"], r["reg_w"])
    return reads, reqs


def region_batch(p, idxs, cig_cap=CIG_CAP):
    """The records and tasks bmh_region_cigar_batch takes for the regions idxs, as host/reg2cigar_batch.c lays them out:
    (readpool, opool_bytes, reqs, tasks, task_cigar_words)"""
    rs = regions()
    reqs, tasks, rpool = np.zeros(len(idxs), dtype=REGION_REQ), [], []
    rb_ = ob_ = slot_ = 0
    for j, i in enumerate(idxs):
        r = rs[i]
        ql, tl = len(r["read"]), r["re"] - r["rb"]
        band, slot, n = plan(p, ql, tl, r["truesc"], r["reg_w"])
        cap = min(ql + tl + 2, cig_cap)
        reqs[j] = (rb_, r["rb"], ob_, ql, tl, r["truesc"], [(-1 if s < 0 else len(tasks) + s) for s in slot])
        made = 0
        for t_ in range(3):
            if slot[t_] == made:
                g = np.zeros((), kswlib.GLB_TASK)
                g["q_off"], g["t_off"], g["qlen"], g["tlen"], g["w"], g["cigar_off"], g["cigar_cap"] = ob_, ob_ + ql, ql, tl, band[t_], slot_, cap
                slot_ += cap
                tasks.append(g)
                made += 1
        rpool.append(r["read"])
        rb_ += ql
        ob_ += ql + tl
    tasks = np.array(tasks, dtype=kswlib.GLB_TASK) if tasks else np.zeros(0, dtype=kswlib.GLB_TASK)
    return np.concatenate(rpool + [np.zeros(0, np.uint8)]), ob_, reqs, tasks, slot_ + 4
