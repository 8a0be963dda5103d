"""Sequence pools past 4 GiB by relocation (plain numpy).

A batch is generated, and its expected results computed by the oracle, on an ordinary small pool.  The same bytes are then put at
a base B inside a large pool and B is added to every q_off / t_off: whatever reads the large pool must return the small pool's
results bit for bit.  So that more than one sequence lies across the boundary, the small pool is laid out as

    [ far | low | S | high ]

with S a string of a few kilobases whose centre is what a placement puts on the boundary.  `low` and `high` are ordinary generated
batches (wholly below / above it); two families of tasks VIEW slices of S that cross its centre: family T takes its target from S
(forwards, and with BMH_F_TREV walking down across the boundary) and a related query from `far`, family Q the converse.  The
crossing falls on the first base, on the last base and on every residue mod 8 of the row / column index.

Decoy: wherever a byte of the block sits at an offset x that a truncated offset (x mod 2^32, for the 2^33 placement also
x mod 2^33) would not reach, the large pool holds at the truncated offset a different valid base code.  A reader that drops the
high word then reads in bounds, plausible, wrong bases, and is caught by a result, not by a fault."""
import numpy as np

import kswgen
from kswlib import BMH_F_QREV, BMH_F_TREV, BMH_F_TPAC, BMH_F_QCOMP, EXT_TASK, GLB_TASK, SW_TASK, SEED_TASK

TWO32 = 1 << 32
S_LEN = 8192
PAD = 1 << 16                                    # zero bytes kept in front of every large pool (see relocate)
BIT31_BASE = TWO32 + (1 << 31) + 12345           # odd; the low word of every offset has bit 31 set
PLACEMENTS = ("straddle32", "bit31", "straddle33")
BOUNDARY = {"straddle32": TWO32, "bit31": None, "straddle33": 2 * TWO32}
MASKS = {"straddle32": (TWO32 - 1,), "bit31": (TWO32 - 1,), "straddle33": (TWO32 - 1, 2 * TWO32 - 1)}
ORD, FAM_T, FAM_Q = 0, 1, 2
MIN_VIEWS, MIN_SIDE = 64, 200                    # the caps of every (entry point, kernel family, straddling placement)


def comp(s):
    return np.where(s < 4, 3 - s, 4).astype(np.uint8)


def decoy_of(block):
    """A valid base code that differs from every byte of `block` (an N becomes a base)."""
    b = np.asarray(block, np.uint8)
    k = (np.arange(len(b), dtype=np.int64) * 2654435761 >> 7) % 3 + 1
    return np.where(b < 4, (b + k) & 3, k).astype(np.uint8)


# ---- relocation ------------------------------------------------------------------------------------------------------

def kind_of(tasks):
    return {EXT_TASK: "ext", GLB_TASK: "glb", SW_TASK: "sw", SEED_TASK: "seed"}[tasks.dtype]


def shifted(tasks, base):
    """The tasks with `base` added to every pool offset (not to the t_off of a BMH_F_TPAC task: that is a coordinate)."""
    out = tasks.copy()
    out["q_off"] += np.uint64(base)
    pool_t = np.ones(len(out), bool) if "flags" not in out.dtype.names else (out["flags"] & BMH_F_TPAC) == 0
    out["t_off"][pool_t] += np.uint64(base)
    return out


def segments(pool, base, masks):
    """What the large pool holds, as (offset, bytes) runs in writing order: the decoys first, the block last."""
    pool = np.asarray(pool, np.uint8)
    n, dec, out = len(pool), decoy_of(pool), []
    for m in masks:
        lo = max(base, m + 1)                    # bytes at lo.. have x & m != x
        while lo < base + n:
            hi = min(base + n, (lo // (m + 1) + 1) * (m + 1))
            out.append((lo & m, dec[lo - base:hi - base]))
            lo = hi
    for off, run in out:
        assert off + len(run) <= base or off >= base + n, "a decoy would overwrite the block"
    return out + [(base, pool)]


def relocate(pool, tasks, base, total, masks=(TWO32 - 1,)):
    """(large pool of `total` bytes with `pool` at `base` and its decoys, tasks moved by `base`)."""
    assert base + len(pool) <= total
    # (lazily mapped: only the pages written are ever touched.)  PAD zero bytes in front of offset 0, as the device pools have: a
    # reader that truncates the top offset of a reversed sequence across the boundary walks down past offset 0, and stays in bounds
    big = np.zeros(PAD + total, np.uint8)[PAD:]
    for off, run in segments(pool, base, masks):
        big[off:off + len(run)] = run
    return big, shifted(tasks, base)


# ---- spans and the census --------------------------------------------------------------------------------------------

def spans(tasks):
    """(q_lo, q_hi, q_rev, t_lo, t_hi, t_rev): the half-open byte range of either sequence of every task in the pool."""
    kind = kind_of(tasks)
    qo, to = tasks["q_off"].astype(np.int64), tasks["t_off"].astype(np.int64)
    if kind == "seed":
        ql, tl = tasks["l_query"].astype(np.int64), tasks["wlen"].astype(np.int64)
    else:
        ql, tl = tasks["qlen"].astype(np.int64), tasks["tlen"].astype(np.int64)
    flags = tasks["flags"].astype(np.int64) if "flags" in tasks.dtype.names else np.zeros(len(tasks), np.int64)
    qrev, trev = (flags & BMH_F_QREV) != 0, (flags & BMH_F_TREV) != 0
    if kind == "seed":
        qrev, trev = np.zeros(len(tasks), bool), np.zeros(len(tasks), bool)
    q_lo = np.where(qrev, qo - np.maximum(ql, 1) + 1, qo)
    t_lo = np.where(trev, to - np.maximum(tl, 1) + 1, to)
    return q_lo, q_lo + ql, qrev, t_lo, t_lo + tl, trev


def census(tasks, fam, boundary):
    """Per family the tasks wholly below, across and wholly above `boundary`; for T (Q) the crossing is the target's (query's):
    how many are reversed, and which residues mod 8 the index of the first base on the far side takes."""
    q_lo, q_hi, qrev, t_lo, t_hi, trev = spans(tasks)
    lo, hi = np.minimum(q_lo, t_lo), np.maximum(q_hi, t_hi)
    qx, tx = (q_lo < boundary) & (q_hi > boundary), (t_lo < boundary) & (t_hi > boundary)
    out = {}
    for name, f in (("ord", ORD), ("T", FAM_T), ("Q", FAM_Q)):
        sel = fam == f
        d = dict(n=int(sel.sum()), below=int((sel & (hi <= boundary)).sum()), above=int((sel & (lo >= boundary)).sum()),
                 across=int((sel & (qx | tx)).sum()))
        if f != ORD:
            x, s_lo, s_hi, rev = (tx, t_lo, t_hi, trev) if f == FAM_T else (qx, q_lo, q_hi, qrev)
            x = sel & x
            idx = np.where(rev, s_hi - boundary, boundary - s_lo)[x]       # index of the first base past the boundary
            d.update(across=int(x.sum()), reversed=int((x & rev).sum()), residues=sorted(set((idx % 8).tolist())),
                     first=int((idx == 1).sum()), last=int((idx == (s_hi - s_lo)[x] - 1).sum()))
        out[name] = d
    return out


def assert_caps(c, has_rev=True, what="", edges=True):
    """The caps a straddling placement must meet, so that no comparison passes vacuously.  edges=False for the part of a batch
    that routing sends to one kernel: the crossings on the first and the last base are asked of the whole batch only."""
    for f in ("T", "Q"):
        assert c[f]["across"] >= MIN_VIEWS, f"{what}family {f}: {c[f]['across']} tasks across the boundary"
        assert c[f]["residues"] == list(range(8)), f"{what}family {f}: crossing residues {c[f]['residues']}"
        assert not edges or (c[f]["first"] >= 1 and c[f]["last"] >= 1), f"{what}family {f}: no crossing on the first / last base"
        if has_rev:
            assert 4 * c[f]["reversed"] >= c[f]["across"], f"{what}family {f}: {c[f]['reversed']} of {c[f]['across']} reversed"
    assert c["ord"]["below"] >= MIN_SIDE and c["ord"]["above"] >= MIN_SIDE, f"{what}{c['ord']}"


# ---- the layout --------------------------------------------------------------------------------------------------------

class Views:
    """Slices of S that cross its centre, in the orientation the task will read them."""

    def __init__(self, rng, p_n=0.01):
        self.rng, self.S, self.k = rng, kswgen.rand_seq(rng, S_LEN, p_n), {}

    def cut(self, n, rev, fam=0):
        """(offset of base 0 relative to S, the n bases as read) of family `fam`'s next crossing slice: `idx` bases lie before the
        centre -- 1, n - 1, then every residue mod 8 in turn, forwards and reversed alike."""
        assert 9 <= n <= S_LEN // 2
        k, c = self.k.get(fam, 0), S_LEN // 2
        self.k[fam] = k + 1
        idx = 1 if k < 2 else n - 1 if k < 4 else 1 + ((int(self.rng.integers(0, n - 8)) & ~7) + (k // 2) % 8 - 1) % (n - 1)
        if rev:   # base 0 at the top, idx bases at or above the centre
            top = c + idx - 1
            return top, self.S[top - n + 1:top + 1][::-1].copy()
        return c - idx, self.S[c - idx:c - idx + n].copy()


class Batch:
    """One relocatable batch: pool, tasks, the family of every task, and the small-pool offset the boundary falls on."""

    def __init__(self, views, far, view_tasks, s_field, low, high, extra=None):
        """far: PoolBuilder of the view tasks' other sequences, its tasks holding S-relative offsets in the field s_field[k];
        low / high: (pool, tasks) batches; extra: further (pool, tasks) stored above `high`."""
        dtype = low[1].dtype
        fpool = np.concatenate(far.chunks) if far.chunks else np.zeros(0, np.uint8)
        vt = np.array(view_tasks, dtype=dtype)
        parts, tasks, fam = [], [], []
        s_off = len(fpool) + len(low[0])
        for k in range(len(vt)):
            a, b = ("q_off", "t_off") if s_field[k] == "q" else ("t_off", "q_off")
            vt[a][k] += s_off
        parts.append(fpool), tasks.append(vt), fam.append(np.where(np.array(s_field) == "t", FAM_T, FAM_Q).astype(np.uint8))
        off = len(fpool)
        layout = [low, (views.S, np.zeros(0, dtype)), high] + ([extra] if extra is not None else [])
        for pool, t in layout:
            t = t.copy()
            t["q_off"] += np.uint64(off)
            if "flags" in t.dtype.names:
                sel = (t["flags"] & BMH_F_TPAC) == 0
                t["t_off"][sel] += np.uint64(off)
            else:
                t["t_off"] += np.uint64(off)
            parts.append(np.asarray(pool, np.uint8)), tasks.append(t), fam.append(np.zeros(len(t), np.uint8))
            off += len(pool)
        self.pool = np.concatenate(parts + [np.zeros(8, np.uint8)])
        self.tasks, self.fam = np.concatenate(tasks), np.concatenate(fam)
        self.center = s_off + S_LEN // 2
        self.kind = kind_of(self.tasks)
        self.words = 0
        if self.kind == "glb":                   # CIGAR slots one after the other
            caps = self.tasks["cigar_cap"].astype(np.int64)
            self.tasks["cigar_off"] = np.concatenate([[0], np.cumsum(caps)[:-1]])
            self.words = int(caps.sum())

    def base(self, placement):
        return BIT31_BASE if placement == "bit31" else BOUNDARY[placement] - self.center

    def total(self, placement):
        return self.base(placement) + len(self.pool)

    def moved(self, placement):
        return shifted(self.tasks, self.base(placement))

    def segments(self, placement):
        return segments(self.pool, self.base(placement), MASKS[placement])

    def relocate(self, placement, total=None):
        return relocate(self.pool, self.tasks, self.base(placement), total or self.total(placement), MASKS[placement])

    def census(self, placement):
        b = BOUNDARY[placement]
        return census(self.moved(placement), self.fam, b if b is not None else TWO32)

    def truncated(self, placement, mask=TWO32 - 1):
        """The moved tasks as a reader that drops the high word sees them (for showing on the CPU that the inputs discriminate)."""
        t = self.moved(placement)
        t["q_off"] &= np.uint64(mask)
        t["t_off"] &= np.uint64(mask)
        return t


def _sub(rng, s, rate=0.03):
    s = s.copy()
    m = (rng.random(len(s)) < rate) & (s < 4)
    s[m] = (s[m] + rng.integers(1, 4, int(m.sum()))) & 3
    return s


def _related(rng, x, n, max_indel=8):
    """About n bases related to the start of x: substitutions and, half of the time, one indel."""
    y = _sub(rng, np.where(x[:n] < 4, x[:n], 0).astype(np.uint8))
    if len(y) > 24 and rng.random() < 0.5:
        c, d = int(rng.integers(8, len(y) - 8)), int(rng.integers(1, max_indel + 1))
        y = np.concatenate([y[:c], y[c + d:]]) if rng.random() < 0.5 else np.concatenate([y[:c], kswgen.rand_seq(rng, d), y[c:]])
    return y if len(y) else kswgen.rand_seq(rng, 1)


EXT_QLENS = (20, 30, 50, 64, 80, 96, 110, 128, 160, 250, 300, 500, 540)   # every bin of the dispatcher, both halves of bin 2


def ext_batch(rng, n_side=1200, n_views=104, read_len=(100, 560), qlens=EXT_QLENS, tail=(20, 120), long_targets=0):
    """kswgen.gen_ext_realistic(hard=True) below and above, and families T and Q over S.  long_targets: that many ordinary tasks
    above whose target is longer than the group kernels' LDS stage (kGrpTcapHost = 1024)."""
    v, far, vt, sf = Views(rng), kswgen.PoolBuilder(EXT_TASK), [], []
    for k in range(2 * n_views):
        ql, fam_t = int(qlens[(k // 2) % len(qlens)]), k % 2 == 0
        rev, orev = bool((k // 2) % 2), bool(rng.random() < 0.3)
        if fam_t:
            tl = ql + int(rng.integers(*tail))
            to, t = v.cut(tl, rev, 1)
            q = _related(rng, t, ql)[:ql]
            q[rng.random(len(q)) < 0.02] = 4
            qo = far.put(q, orev)
            flags = (BMH_F_TREV if rev else 0) | (BMH_F_QREV if orev else 0)
            sf.append("t")
        else:
            qo, q = v.cut(ql, rev, 2)
            t = np.concatenate([_related(rng, q, ql), kswgen.rand_seq(rng, int(rng.integers(*tail)))])
            to = far.put(t, orev)
            flags = (BMH_F_QREV if rev else 0) | (BMH_F_TREV if orev else 0)
            sf.append("q")
        h0 = int(rng.integers(19, 200))
        vt.append((qo, to, len(q), len(t), h0, int(rng.choice([20, 100])), 5, flags, 0))
    low = kswgen.gen_ext_realistic(rng, n_side, read_len=read_len, hard=True)
    high = kswgen.gen_ext_realistic(rng, n_side, read_len=read_len, hard=True)
    extra = None
    if long_targets:
        pb = kswgen.PoolBuilder(EXT_TASK)
        for _ in range(long_targets):
            ql = int(rng.integers(20, 250))
            q, t = kswgen.flank_pair(rng, ql, int(rng.integers(1100, 1600)))
            kswgen._add_ext(pb, rng, q, t, int(rng.integers(19, 150)), 100, 5)
        extra = pb.finish()
    return Batch(v, far, vt, sf, low, high, extra)


def _glb_w(rng, q, t, wclass):
    d = abs(len(q) - len(t))
    return d + int(rng.integers(0, 6)) if wclass == 0 else max(d, int(rng.integers(*wclass)))


GLB_WCLASSES = (0, (8, 32), (32, 48), (48, 64), (64, 130))    # tight, the three lane kernels, the wave kernel


def glb_batch(rng, n_side=400, n_views=80, read_len=(100, 560), view_len=(9, 560), wclasses=GLB_WCLASSES, realistic=True, extra=None,
              n_class=None):
    """kswgen's global generators below and above, families T and Q over S (ksw_global2 tasks carry no flags: forwards only).
    Besides the realistic regions each side holds n_class regions (default: a quarter of n_side, taken from it) whose bands
    cycle through wclasses like the views'; realistic=False: only those; extra: a further (pool, tasks) batch stored above."""
    v, far, vt, sf = Views(rng), kswgen.PoolBuilder(GLB_TASK), [], []
    for k in range(2 * n_views):
        n, fam_t = int(rng.integers(view_len[0], view_len[1] + 1)), k % 2 == 0
        so, x = v.cut(n, False, k % 2)
        y = _related(rng, x, n)
        if not fam_t:
            y[rng.random(len(y)) < 0.01] = 4
        oo = far.put(y)
        q, t = (y, x) if fam_t else (x, y)
        w = _glb_w(rng, q, t, wclasses[(k // 2) % len(wclasses)])
        vt.append((oo, so, len(q), len(t), w, 0, len(q) + len(t) + 2) if fam_t else (so, oo, len(q), len(t), w, 0, len(q) + len(t) + 2))
        sf.append("t" if fam_t else "q")

    def side():
        n_cls = n_class if n_class is not None else n_side // 4 if realistic else n_side
        pb = kswgen.PoolBuilder(GLB_TASK)       # every band class, short regions too
        for k in range(n_cls):
            n = int(rng.integers(view_len[0], view_len[1] + 1))
            q = kswgen.rand_seq(rng, n, 0.01)
            t = _related(rng, q, n)
            kswgen._add_glb(pb, q, t, _glb_w(rng, q, t, wclasses[k % len(wclasses)]), rng.random() < 0.9)
        b = kswgen.finish_glb(pb)
        if not realistic:
            return b[0], b[1]
        a = kswgen.gen_glb_realistic(rng, n_side - (0 if n_class is not None else n_cls), read_len=read_len, hard=True)
        tb = b[1].copy()
        tb["q_off"] += len(a[0])
        tb["t_off"] += len(a[0])
        return np.concatenate([a[0], b[0]]), np.concatenate([a[1], tb])
    return Batch(v, far, vt, sf, side(), side(), extra)


def sw_batch(rng, p, n_side=300, n_views=80, qlen=(30, 300), flank=(20, 400), xtra=None, side=None):
    """Mate-rescue shaped ksw_align2 tasks below and above (queries with an N, reversed and complemented mates among them), and
    families T and Q over S.  xtra(qlen): the task's xtra word, bwa's by default."""
    xtra = xtra or (lambda n: kswgen.sw_xtra_bwa(p, n))
    v, far, vt, sf = Views(rng), kswgen.PoolBuilder(SW_TASK), [], []
    for k in range(2 * n_views):
        ql, fam_t = int(rng.integers(qlen[0], qlen[1] + 1)), k % 2 == 0
        rev, orev, qcomp = bool((k // 2) % 2), bool(rng.random() < 0.3), bool(rng.random() < 0.3)
        if fam_t:
            a, b = int(rng.integers(*flank)), int(rng.integers(*flank))
            to, t = v.cut(min(a + ql + b, S_LEN // 2), rev, 1)
            q = _related(rng, t[a:], ql, 4)
            if k % 3 == 0:
                q[int(rng.integers(0, len(q)))] = 4      # the N scan of the query
            qo = far.put(comp(q) if qcomp else q, orev)
            flags = (BMH_F_TREV if rev else 0) | (BMH_F_QREV if orev else 0) | (BMH_F_QCOMP if qcomp else 0)
        else:
            qo, qs = v.cut(ql, rev, 2)                      # S holds the stored form: the complement where QCOMP is set
            q = comp(qs) if qcomp else qs
            t = np.concatenate([kswgen.rand_seq(rng, int(rng.integers(*flank))), _related(rng, q, ql, 4),
                                kswgen.rand_seq(rng, int(rng.integers(*flank)))])
            to = far.put(t, orev)
            flags = (BMH_F_QREV if rev else 0) | (BMH_F_TREV if orev else 0) | (BMH_F_QCOMP if qcomp else 0)
        vt.append((qo, to, len(t), len(q), flags, xtra(len(q)), 0))
        sf.append("t" if fam_t else "q")
    if side is None:
        def side():
            return kswgen.gen_sw_materescue(rng, n_side, p, read_len=qlen, win=(100, 600), hard=True)
    return Batch(v, far, vt, sf, side(), side())


def _flank_edit(rng, seg, max_indel):
    """A flank on the other sequence: substitutions and, half of the time, an indel of up to max_indel bases (what makes a narrow
    band run again at twice the width)."""
    y = _sub(rng, np.where(seg < 4, seg, 0).astype(np.uint8), 0.02)
    if len(y) > 30 and rng.random() < 0.5:
        c, d = int(rng.integers(10, len(y) - 10)), int(rng.integers(1, max_indel + 1))
        y = np.concatenate([y[:c], y[c + d:]]) if rng.random() < 0.5 else np.concatenate([y[:c], kswgen.rand_seq(rng, d), y[c:]])
    return y


def seed_views(rng, v, far, n_views, read_len=(100, 400), slen=25, ctx=(0, 40), max_indel=12):
    """Fused per-seed records whose read (family Q) or reference window (family T) is a slice of S: the offsets the kernels
    derive for the left and right extensions then cross the boundary as well."""
    vt, sf = [], []
    for k in range(2 * n_views):
        fam_t = k % 2 == 0
        L = int(rng.integers(read_len[0], read_len[1] + 1))
        c0, c1 = int(rng.integers(ctx[0], ctx[1] + 1)), int(rng.integers(ctx[0], ctx[1] + 1))
        so, x = v.cut(L + (c0 + c1 if fam_t else 0), False, k % 2)
        core = x[c0:len(x) - c1] if fam_t else x
        core = core.copy()
        b = int(rng.integers(0, len(core) - slen + 1))
        if k % 16 == 2:
            b = 0                                        # no left extension
        if k % 16 == 4:
            b = len(core) - slen                         # no right extension
        left, seed, right = core[:b], core[b:b + slen], core[b + slen:]
        if fam_t and (seed > 3).any():
            seed = np.where(seed < 4, seed, 0).astype(np.uint8)
        oleft, oright = _flank_edit(rng, left, max_indel), _flank_edit(rng, right, max_indel)
        oseed = np.where(seed < 4, seed, 0).astype(np.uint8)
        if fam_t:   # the window is S's; the read is made from it
            read = np.concatenate([oleft, oseed, oright])
            qo = far.put(read)
            vt.append((qo, so, len(read), len(oleft), slen, c0 + b, len(x), 0, 0))
        else:       # the read is S's; the window is made from it
            e0, e1 = kswgen.rand_seq(rng, c0), kswgen.rand_seq(rng, c1)
            win = np.concatenate([e0, oleft, oseed, oright, e1])
            to = far.put(win)
            vt.append((so, to, len(x), b, slen, c0 + len(oleft), len(win), 0, 0))
        sf.append("t" if fam_t else "q")
    return vt, sf


def seed_side(rng, n, read_len=(100, 400), **kw):
    """Ordinary fused per-seed records of the same make, each with a read and a window of its own."""
    pb = kswgen.PoolBuilder(SEED_TASK)

    class Own:   # a Views stand-in that hands out fresh sequences
        def cut(self, n, rev, fam=0):
            return pb.put(kswgen.rand_seq(rng, n, 0.005)), pb.chunks[-1]
    vt, _ = seed_views(rng, Own(), pb, (n + 1) // 2, read_len, **kw)
    pb.tasks = vt
    return pb.finish()


def seed_batch(rng, n_side=400, n_views=80, read_len=(100, 400), sides=None):
    """sides: (low, high) batches of seeds, e.g. from the package's task generator; default: seed_side()."""
    v, far = Views(rng, p_n=0.0), kswgen.PoolBuilder(SEED_TASK)
    vt, sf = seed_views(rng, v, far, n_views, read_len)
    low, high = sides if sides is not None else (seed_side(rng, n_side, read_len), seed_side(rng, n_side, read_len))
    return Batch(v, far, vt, sf, low, high)
