"""An exact FM-index, in bwa's own format, of a periodic genome -- built in numpy in minutes, without `bwa index`, for
any size up to and past hg38's 2^32 rows, with its whole suffix array known in closed form.

The genome is pac = P^m with P = W.rc(W) for a random word W: P is its own reverse complement, so bwa's text
pac.rc(pac) is P^M with M = 2m -- periodic, and closed under reverse complement as bidirectional SMEM search needs.
Its suffix order follows from the suffix array of the 2p+1 symbols P.P.$ (p = |P|):

  * a position r < p stands for rotation group r: the suffixes r + j*p at least p long (M of them for r = 0, M-1
    otherwise), shortest first (a suffix that is a prefix of another, followed by $, sorts before it);
  * a position p + r, r >= 1, stands for the single tail suffix r + (M-1)*p, shorter than p;
  * position p (the suffix P$) is group 0's shortest member, already counted there; position 2p is the $ row.

Rows of the BWT therefore come in one run per entry of that suffix array, each a single symbol: P[(r-1) mod p] for
group / tail r, with the $ taken out at `primary` (group 0's longest member, the whole text).  From the runs this
module writes what bwa keeps (bwt.h:45-57, bwtindex.c bwt_bwtupdate_core, bwt.c bwt_cal_sa): primary, L2[5], seq_len,
the BWT words with four u64 occurrence counts interleaved before every 128 symbols, and the sampled suffix array
(sa_intv 32, sa[0] = (uint64_t)-1); `write_files` adds .bwt/.sa/.pac/.ann/.amb.  Nothing here runs on a GPU."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U64_MAX = np.uint64(0xffffffffffffffff)
SA_INTV = 32
# hg38-like default: l_pac = m * p = 3.1e9, every read drawn from P^inf occurs 2m = 500 times
BIG_HALF, BIG_M = 6_200_000, 250


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def make_period(rng, half, lead_t=8):
    """P = W.rc(W) for a random W of `half` bases that starts with `lead_t` T's (so that rotation 0 -- the whole text's
    group -- sorts near the end and `primary` lies high).  Redrawn until P is primitive."""
    while True:
        w = rng.integers(0, 4, half).astype(np.uint8)
        w[:min(lead_t, half)] = 3
        P = np.concatenate([w, (3 - w[::-1]).astype(np.uint8)])
        if is_primitive(P):
            return P


def is_primitive(P):
    p = len(P)
    return all(not np.array_equal(P, np.roll(P, d)) for d in range(1, p // 2 + 1) if p % d == 0)


def suffix_array_pp(P):
    """Suffix array of P.P.$ (2p+1 symbols, $ smallest): prefix doubling that re-sorts only unresolved groups, and stops
    as soon as the only ties left are the pairs (r, p+r) -- P[r:].P.$ and P[r:].$ -- where the shorter sorts first."""
    P = np.ascontiguousarray(P, dtype=np.uint8)
    p = len(P)
    N = 2 * p + 1
    s = np.zeros(N + 21, dtype=np.uint64)
    s[:p] = P + 1
    s[p:2 * p] = P + 1  # s[2p] = $ = 0, and zeros past it: $ is unique, so nothing compares beyond it
    key = np.zeros(N, dtype=np.uint64)
    for j in range(21):  # the first 21 symbols, 3 bits each
        key = (key << np.uint64(3)) | s[j:j + N]
    del s
    sa = np.argsort(key, kind="stable").astype(np.int64)
    ks = key[sa]
    del key
    head = np.ones(N, dtype=bool)  # head[i]: sa[i] starts a group
    head[1:] = ks[1:] != ks[:-1]
    del ks
    idx = np.arange(N, dtype=np.int64)
    rank = np.empty(N, dtype=np.int64)
    rank[sa] = np.maximum.accumulate(np.where(head, idx, 0))  # rank = start of the group in sa
    del idx
    h = 21
    while True:
        single = head.copy()
        single[:-1] &= head[1:]
        unres = np.nonzero(~single)[0]  # indices of sa in groups of two or more
        del single
        if len(unres) == 0:
            break
        pos = sa[unres]
        starts = unres[head[unres]]
        if len(unres) == 2 * len(starts):  # every group a pair: is each one (r, p+r)?
            a, b = sa[starts], sa[starts + 1]
            lo, hi = np.minimum(a, b), np.maximum(a, b)
            if ((hi - lo == p) & (lo < p)).all():
                sa[starts], sa[starts + 1] = hi, lo
                break
        nxt = pos + h
        second = np.where(nxt < N, rank[np.minimum(nxt, N - 1)] + 1, 0)
        comp = (rank[pos].astype(np.uint64) << np.uint64(32)) | second.astype(np.uint64)
        order = np.argsort(comp, kind="stable")
        cs = comp[order]
        new = np.ones(len(unres), dtype=bool)
        new[1:] = cs[1:] != cs[:-1]
        pos = pos[order]
        sa[unres] = pos
        head[unres] = new
        rank[pos] = np.maximum.accumulate(np.where(new, unres, 0))
        h *= 2
    return sa


class PeriodicIndex:
    """The FM-index of pac = P^m (both strands: text P^(2m)).  Attributes: P, p, m, M = 2m, l_pac, seq_len, primary,
    L2 (5 ints), bwt (uint32 words, bwa's layout), sa_intv, sa (sampled, sa[0] = UINT64_MAX), contigs [(name, offset,
    len)].  chunk_blocks: 128-symbol blocks per unit of work (small values exercise the chunk seams in tests)."""

    def __init__(self, P, m, n_contigs=1, chunk_blocks=1 << 18, threads=None):
        P = np.ascontiguousarray(P, dtype=np.uint8)
        assert is_primitive(P) and m >= 1
        self.P, self.p, self.m = P, len(P), int(m)
        p, M = self.p, 2 * self.m
        self.M, self.l_pac = M, self.m * p
        self.seq_len = n = M * p
        self.sa_intv = SA_INTV
        threads = threads or _threads()
        spp = suffix_array_pp(P)
        spp = spp[spp != p]  # P$ is group 0's shortest member
        cnt = np.where(spp == 2 * p, 1, np.where(spp > p, 1, np.where(spp == 0, M, M - 1))).astype(np.int64)
        # the BWT symbol of every row of an entry: T[SA - 1], SA = r + j*p (r >= 1) or the tail r + (M-1)*p -> P[r-1];
        # group 0 and the $ row -> P[p-1]
        r = np.where(spp > p, spp - p, spp)
        r = np.where(spp == 2 * p, 0, r)
        self._e = spp
        self._sym = P[(r - 1) % p].astype(np.uint8)
        self._row0 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)  # first row of every entry; [-1] = n + 1
        assert self._row0[-1] == n + 1
        g0 = int(np.nonzero(spp == 0)[0][0])
        self.primary = int(self._row0[g0 + 1] - 1)  # group 0's longest member: SA = 0
        # the stream without $: group 0's run is one shorter
        scnt = cnt.copy()
        scnt[g0] -= 1
        self._s0 = np.concatenate([[0], np.cumsum(scnt)]).astype(np.int64)
        assert self._s0[-1] == n
        # occurrences of every symbol before every run (for the counts at block starts)
        self._cc = np.zeros((len(scnt) + 1, 4), dtype=np.uint64)
        for c in range(4):
            self._cc[1:, c] = np.cumsum(np.where(self._sym == c, scnt, 0))
        tot = self._cc[-1]
        self.L2 = [0] + [int(x) for x in np.cumsum(tot)]
        assert self.L2[4] == n
        self._build_bwt(chunk_blocks, threads)
        self._build_sa(chunk_blocks * 4, threads)
        step = -(-self.l_pac // max(1, int(n_contigs)))
        self.contigs = [("chr%d" % (k + 1), o, min(step, self.l_pac - o)) for k, o in enumerate(range(0, self.l_pac, step))]

    # ---- the BWT words ----
    def _symbols(self, a, z):
        """The $-free BWT symbols [a, z) as uint8."""
        j0 = int(np.searchsorted(self._s0, a, "right")) - 1
        j1 = int(np.searchsorted(self._s0, z, "left"))
        st = np.maximum(self._s0[j0:j1], a)
        en = np.minimum(self._s0[j0 + 1:j1 + 1], z)
        return np.repeat(self._sym[j0:j1], en - st)

    def _counts_at(self, x):
        """Occurrences of each symbol in the stream before positions x (sorted int64 array) -> (len(x), 4) uint64."""
        j = np.searchsorted(self._s0, x, "right") - 1
        part = (x - self._s0[j]).astype(np.uint64)
        out = self._cc[j].copy()
        sym = self._sym[np.minimum(j, len(self._sym) - 1)]
        for c in range(4):
            out[:, c] += np.where((sym == c) & (j < len(self._sym)), part, np.uint64(0))
        return out

    def _build_bwt(self, chunk_blocks, threads):
        n = self.seq_len
        nb = -(-n // 128)
        self.bwt_size = nb * 8 + -(-n // 16) + 8
        words = np.zeros(self.bwt_size, dtype=np.uint32)

        def one(b0):
            b1 = min(b0 + chunk_blocks, nb)
            a, z = b0 * 128, min(b1 * 128, n)
            s = self._symbols(a, z)
            nw = -(-len(s) // 16)
            s = np.concatenate([s, np.zeros(nw * 16 - len(s), np.uint8)]).reshape(-1, 4)
            by = (s[:, 0] << 6) | (s[:, 1] << 4) | (s[:, 2] << 2) | s[:, 3]  # 4 symbols a byte, the first in the top bits
            sw = by.view(">u4").astype(np.uint32)  # 16 a word, the first in the top bits
            cnt = self._counts_at(np.arange(b0, b1, dtype=np.int64) * 128).view(np.uint32).reshape(-1, 8)
            base = b0 * 16
            full = (z - a) // 128  # whole blocks of the chunk
            if full:
                blk = words[base:base + full * 16].reshape(full, 16)
                blk[:, :8] = cnt[:full]
                blk[:, 8:] = sw[:full * 8].reshape(full, 8)
            if full < b1 - b0:  # the last, partial block
                at = base + full * 16
                words[at:at + 8] = cnt[full]
                words[at + 8:at + 8 + nw - full * 8] = sw[full * 8:]

        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(0, nb, chunk_blocks)))
        words[-8:] = self._counts_at(np.array([n], dtype=np.int64)).view(np.uint32).reshape(8)  # the last element: the totals
        self.bwt = words

    # ---- the suffix array ----
    def sa_of(self, k):
        """bwt_sa of rows k (array-like, 0..seq_len) in closed form.  Row 0 (the $ suffix) gives what bwt_sa gives there:
        sa[0] = (uint64_t)-1, not seq_len (bwt.c:82)."""
        k = np.asarray(k, dtype=np.int64)
        j = np.searchsorted(self._row0, k, "right") - 1
        e, o = self._e[j], k - self._row0[j]
        p, M = self.p, self.M
        sa = np.where(e == 2 * p, -1, np.where(e > p, e - p + (M - 1) * p,
                                                         np.where(e == 0, (M - 1 - o) * p, e + (M - 2 - o) * p)))
        return sa.astype(np.uint64)

    def row_of(self, i):
        """The row whose suffix starts at text position i (array-like, 0..seq_len-1): the inverse of sa_of."""
        i = np.asarray(i, dtype=np.int64)
        if not hasattr(self, "_inv"):
            self._inv = np.empty(2 * self.p + 1, dtype=np.int64)
            self._inv[self._e] = np.arange(len(self._e))
        p, M = self.p, self.M
        r, j = i % p, i // p
        tail = (j == M - 1) & (r > 0)
        ent = self._inv[np.where(tail, p + r, r)]
        return (self._row0[ent] + np.where(tail, 0, M - 1 - (r > 0) - j)).astype(np.uint64)

    def _build_sa(self, chunk, threads):
        n_sa = (self.seq_len + SA_INTV) // SA_INTV
        sa = np.empty(n_sa, dtype=np.uint64)

        def one(i0):
            i1 = min(i0 + chunk, n_sa)
            sa[i0:i1] = self.sa_of(np.arange(i0, i1, dtype=np.int64) * SA_INTV)

        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(0, n_sa, chunk)))
        self.n_sa, self.sa = n_sa, sa

    # ---- closed-form answers ----
    def occurrences(self, r0, length):
        """Every start of the substring of P^inf at offset r0 (mod p), `length` long, in the text P^M (doubled
        coordinates), assuming it occurs nowhere else."""
        r0 = int(r0) % self.p
        last = self.seq_len - int(length)
        return np.arange(r0, last + 1, self.p, dtype=np.uint64) if last >= r0 else np.zeros(0, np.uint64)

    def substring(self, r0, length):
        """length bases of P^inf from offset r0."""
        r0 = int(r0) % self.p
        reps = -(-(r0 + int(length)) // self.p)
        return np.tile(self.P, reps)[r0:r0 + int(length)].copy()

    def raw(self):
        """(primary, L2, seq_len, bwt words, sa_intv, sa): what Context.set_bwt and kswlib.make_cbwt take."""
        return self.primary, list(self.L2), self.seq_len, self.bwt, self.sa_intv, self.sa

    def pac_bytes(self):
        """The .pac file: l_pac 2-bit codes, four a byte, the first in the top bits, then bwa's trailer (bntseq.c:277-285)."""
        p, m = self.p, self.m

        def pack(codes):
            c = np.concatenate([codes, np.zeros(-len(codes) % 4, np.uint8)]).reshape(-1, 4)
            return ((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8)

        parts = [np.tile(pack(np.tile(self.P, 4)), m // 4)] if m >= 4 else []
        if m % 4:
            parts.append(pack(np.tile(self.P, m % 4)))
        body = np.concatenate(parts)
        assert len(body) == -(-self.l_pac // 4)
        tail = [0] if self.l_pac % 4 == 0 else []
        return np.concatenate([body, np.array(tail + [self.l_pac % 4], np.uint8)])

    def write_files(self, prefix):
        """<prefix>.bwt/.sa/.pac/.ann/.amb as `bwa index` writes them (bwt_dump_bwt, bwt_dump_sa, bns_dump)."""
        hdr = np.array([self.primary] + self.L2[1:], dtype=np.uint64)
        with open(prefix + ".bwt", "wb") as f:
            hdr.tofile(f)
            self.bwt.tofile(f)
        with open(prefix + ".sa", "wb") as f:
            np.concatenate([hdr, np.array([self.sa_intv, self.seq_len], np.uint64)]).tofile(f)
            self.sa[1:].tofile(f)
        self.pac_bytes().tofile(prefix + ".pac")
        with open(prefix + ".ann", "w") as f:
            f.write("%d %d %u\n" % (self.l_pac, len(self.contigs), 11))
            for name, off, ln in self.contigs:
                f.write("0 %s (null)\n%d %d 0\n" % (name, off, ln))
        with open(prefix + ".amb", "w") as f:
            f.write("%d %d 0\n" % (self.l_pac, len(self.contigs)))


def big(seed=2024):
    """The hg38-sized index: l_pac 3.1e9, seq_len 6.2e9, with seq_len, L2[3] and primary all past 2^32."""
    rng = np.random.default_rng(seed)
    ix = PeriodicIndex(make_period(rng, BIG_HALF), BIG_M, n_contigs=16)
    assert ix.seq_len > 1 << 32 and ix.L2[3] > 1 << 32 and ix.primary > 1 << 32
    assert all(ln < 1 << 31 for _, _, ln in ix.contigs)
    return ix
