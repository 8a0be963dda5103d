"""The FM-index kernels on an hg38-sized index: 6.2e9 rows, with seq_len, primary, L2[3], the suffix-array values and the
interval starts x0/x1 past 2^32 (tests/periodic_index.py: pac = P^250, p = 12.4e6, an exact bwa-format index whose
suffix array is known in closed form).  bmh_sa_batch, bmh_smem_batch (both kernels), bmh_seed_batch and
bmh_seed_chain_batch against the closed form, the oracle and the host chainer; and the device index cache of
bmh_ctx_set_bwt when a new index is built at the addresses of a freed one."""
import numpy as np
import pytest

import kswlib
import periodic_index as pi
from __graft_entry__ import load_package
from test_chain_cpu import CHAIN_OPT
from test_chain_gpu import _assert_same, _host_chains, _smem_opt
from test_fmindex_cpu import _same_calls
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xffffffffffffffff)
TWO32 = 1 << 32
KERNELS = ["conv", "loops"]


def _opt():
    """mem_opt_t's defaults (bwamem.c mem_opt_init) as bmh_smem_opt_t: min_seed_len 19, split_factor 1.5, split_width 10."""
    o = np.zeros((), dtype=kswlib.SMEM_OPT)
    o["min_seed_len"], o["split_len"], o["split_width"], o["start_width"] = 19, 29, 10, 1
    return o


def _chain_opt(max_occ):
    o = np.zeros((), dtype=CHAIN_OPT)
    o["w"], o["max_chain_gap"], o["min_seed_len"], o["max_occ"] = 100, 10000, 19, max_occ
    o["split_len"], o["split_width"], o["mask_level"], o["chain_drop_ratio"] = 29, 10, 0.5, 0.5
    return o


# ---- the device index cache: a smaller index built where a freed one lay ---------------------------------------------------

def test_set_bwt_uploads_a_new_index_built_at_the_old_addresses():
    """Index A in the front of a buffer, bound and its context closed; index B, strictly smaller, written over it at the same
    addresses and bound on a new context.  A cache keyed on the host pointers alone hands B's context A's device copy and
    A's shape: every answer below would be A's (and no access would leave A's allocation, A being the larger)."""
    rng = np.random.default_rng(41)
    A = pi.PeriodicIndex(pi.make_period(rng, 3001), 7)
    B = pi.PeriodicIndex(pi.make_period(rng, 2003), 5)
    assert B.bwt_size < A.bwt_size and B.n_sa < A.n_sa and B.seq_len < A.seq_len
    words = np.zeros(A.bwt_size, dtype=np.uint32)
    samp = np.zeros(A.n_sa, dtype=np.uint64)
    opt = _opt()

    def bind(ix):
        words[:ix.bwt_size], samp[:ix.n_sa] = ix.bwt, ix.sa
        ctx = _ctx_with({})
        ctx.set_bwt(ix.primary, ix.L2, ix.seq_len, words[:ix.bwt_size], ix.sa_intv, samp[:ix.n_sa])
        return ctx

    def check(ctx, ix):
        keep = []
        cb = kswlib.make_cbwt(*ix.raw(), keep)
        ks = np.concatenate([np.arange(0, ix.seq_len + 1, 7), [ix.primary, ix.seq_len]]).astype(np.uint64)
        got = ctx.sa_batch(ks)
        assert (got == ix.sa_of(ks)).all()
        assert (got[:500] == kswlib.orc_sa(cb, ks[:500])).all()
        reads = [ix.substring(int(r0), int(L)) for r0, L in zip(rng.integers(0, ix.p, 300), rng.choice([20, 75, 150], 300))]
        calls = ctx.smem_batch(opt, reads)
        for k, rd in enumerate(reads):
            assert _same_calls(calls[k], kswlib.orc_smem_calls(cb, opt, rd)), f"read {k}"
        return calls

    ctx = bind(A)
    check(ctx, A)
    ctx.close()
    ctx = bind(B)
    calls = check(ctx, B)
    assert all(len(c) and int(v["x2"][0]) in (B.M, B.M - 1) for c, v in calls)  # whole-copy intervals: B's 2m, not A's
    ctx.close()


# ---- the hg38-sized index --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """ONE big index per process: generated here (about a minute), resident on the device for the module."""
    ix = pi.big()
    keep = []
    cb = kswlib.make_cbwt(*ix.raw(), keep)
    ctx = _ctx_with({})
    ctx.set_bwt(*ix.raw())
    yield ix, cb, ctx
    ctx.close()
    del keep[:]


def _edge_rows(ix):
    e = [0, 1, 2, 31, 32, 33, ix.primary - 1, ix.primary, ix.primary + 1, ix.seq_len - 1, ix.seq_len,
         TWO32 - 1, TWO32, TWO32 + 1]
    for d in range(-4, 5):  # sampled rows on both sides of 2^32, and their neighbours
        e += [TWO32 + 32 * d - 1, TWO32 + 32 * d, TWO32 + 32 * d + 1]
    # rows whose LF walk reaches primary (the whole text) before a sampled row: the suffixes at positions 1..40
    e += [int(x) for x in ix.row_of(np.arange(1, 41))]
    # and the last rows of the text's end (tails), the first and last rows of every symbol
    e += [int(x) for x in ix.row_of(np.arange(ix.seq_len - 40, ix.seq_len))]
    e += [v for c in range(4) for v in (ix.L2[c] + 1, ix.L2[c + 1])]
    return np.array(e, dtype=np.uint64)


def test_sa_batch_past_2_32(big):
    ix, cb, ctx = big
    rng = np.random.default_rng(1)
    edges = _edge_rows(ix)
    ks = np.concatenate([edges, rng.integers(0, ix.seq_len + 1, 200_000).astype(np.uint64)])
    got = ctx.sa_batch(ks)
    want = ix.sa_of(ks)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first k={ks[bad[0]]}: {got[bad[0]]} against {want[bad[0]]}"
    assert (want[len(edges):] > np.uint64(TWO32)).mean() > 0.25 and (ks > np.uint64(TWO32)).mean() > 0.25
    sample = np.concatenate([edges, ks[len(edges):len(edges) + 3000]])
    assert (kswlib.orc_sa(cb, sample) == got[:len(sample)]).all()


def _reads(rng, ix, n):
    """Reads of P^inf at 0 / 2 / 12 % mutation, some bridging a period seam (one of their copies then bridges the strands at
    l_pac, past 2^31), with N runs; empty reads; random reads (small intervals)."""
    lens = [1, 19, 20, 150, 151, 300, 600]
    out, r0s = [], []
    for k in range(n):
        L = int(rng.choice(lens))
        kind = k % 10
        if kind in (0, 1):
            out.append(np.zeros(0, np.uint8) if kind == 0 else rng.integers(0, 4, L).astype(np.uint8))
            r0s.append(-1)
            continue
        r0 = ix.p - int(rng.integers(1, L + 1)) if kind in (2, 3) else int(rng.integers(0, ix.p))
        rd = ix.substring(r0, L)
        mut = [0.0, 0.0, 0.02, 0.12][k % 4]
        m = rng.random(L) < mut
        rd[m] = (rd[m] + rng.integers(1, 4, m.sum())) % 4
        if kind == 9:
            at = int(rng.integers(0, L))
            rd[at:at + int(rng.integers(1, 8))] = 4
        out.append(rd)
        r0s.append(r0 if mut == 0 and kind != 9 else -1)
    return out, r0s


@pytest.mark.parametrize("emit", ["all", "min_seed_len"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_smem_batch_past_2_32(big, kernel, emit, monkeypatch):
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    ix, cb, ctx = big
    opt = _opt()
    opt["min_emit_len"] = 0 if emit == "all" else int(opt["min_seed_len"])
    rng = np.random.default_rng(7 + len(kernel) + len(emit))
    reads, _ = _reads(rng, ix, 2000)
    got = ctx.smem_batch(opt, reads)
    n_iv = n_hi = 0
    for r, (g, rd) in enumerate(zip(got, reads)):
        w = kswlib.orc_smem_calls(cb, opt, rd) if len(rd) else (np.zeros(0, kswlib.SMEM_CALL), np.zeros(0, kswlib.SMEM_INTV))
        assert _same_calls(g, w), f"read {r} (len {len(rd)})"
        n_iv += len(g[1])
        n_hi += int(((g[1]["x0"] > np.uint64(TWO32)) | (g[1]["x1"] > np.uint64(TWO32))).sum())
    assert n_iv > (5000 if emit == "all" else 1500) and n_hi > n_iv // 4, (n_iv, n_hi)


@pytest.mark.parametrize("max_occ", ["10000", "2m", "2m-2"])
def test_seed_batch_past_2_32(big, max_occ):
    """Every looked-up interval's positions are bwt_sa of its rows (closed form and bmh_sa_batch); for an unmutated read the
    whole-read interval holds every copy on both strands, {r0 + j*p}; at max_occ = 2m-2 no whole-copy interval is looked up."""
    ix, cb, ctx = big
    mo = {"10000": 10000, "2m": ix.M, "2m-2": ix.M - 2}[max_occ]
    opt = _opt()
    rng = np.random.default_rng(mo)
    reads, r0s = _reads(rng, ix, 1200)
    tables, offs, pos = ctx.seed_batch(opt, mo, reads)
    keys, got, n_whole, n_whole_looked = [], [], 0, 0
    for r, ((c, iv), so) in enumerate(zip(tables, offs)):
        ln = (iv["info"] & np.uint64(0xffffffff)).astype(np.int64) - (iv["info"] >> np.uint64(32)).astype(np.int64)
        look = (ln >= 19) & (iv["x2"] <= np.uint64(mo))
        assert ((so != NONE) == look).all(), f"read {r}"
        for k in np.nonzero(look)[0]:
            x0, x2, b = int(iv["x0"][k]), int(iv["x2"][k]), int(so[k])
            keys.append(np.arange(x0, x0 + x2, dtype=np.uint64))
            got.append(pos[b:b + x2])
        L = len(reads[r])
        if r0s[r] >= 0 and L >= 150:
            whole = np.nonzero(ln == L)[0]
            assert len(whole) == 1, f"read {r}"
            k = int(whole[0])
            occ = ix.occurrences(r0s[r], L)
            assert int(iv["x2"][k]) == len(occ) and len(occ) in (ix.M, ix.M - 1)
            n_whole += 1
            if look[k]:
                n_whole_looked += 1
                b = int(so[k])
                mine = np.sort(pos[b:b + len(occ)])
                # the read's own strand and its reverse complement: P^inf is closed under rc, so both lie in the set
                assert (mine == occ).all(), f"read {r}"
                assert (mine < np.uint64(ix.l_pac)).any() and (mine >= np.uint64(ix.l_pac)).any() and mine[-1] > np.uint64(TWO32)
    assert n_whole > 100
    assert n_whole_looked == (0 if mo == ix.M - 2 else n_whole)
    if mo == ix.M - 2:  # every interval at least min_seed_len long lies in P^inf and covers 2m-1 or 2m copies: none looked up
        assert len(keys) == 0 and len(pos) == 0
        return
    keys, got = np.concatenate(keys), np.concatenate(got)
    assert len(keys) == len(pos) and len(keys) > 1000
    assert (got == ix.sa_of(keys)).all()
    assert (got == ctx.sa_batch(keys)).all()
    assert (got > np.uint64(TWO32)).mean() > 0.2


def test_seed_chain_batch_past_2_32(big):
    """The fused seeding + chaining against bmh_chain_reads on bmh_seed_batch's tables: chains placed past 2^32, seeds that
    bridge the strands at l_pac dropped by both."""
    ix, cb, ctx = big
    rng = np.random.default_rng(3)
    reads, _ = _reads(rng, ix, 600)
    n_hi = n_chains = 0
    for mo in (ix.M, 40):
        o = _chain_opt(mo)
        tables, offs, sa_pos = ctx.seed_batch(_smem_opt(o), mo, reads)
        want = _host_chains(load_package().lib(), o, ix.l_pac, reads, list(tables), offs, sa_pos)
        got = ctx.seed_chain_batch(_smem_opt(o), o, ix.l_pac, reads)
        _assert_same(got, want, f"max_occ={mo}")
        for chains in got:
            for sd in chains:
                rb = sd["rbeg"].astype(np.int64)
                assert not ((rb < ix.l_pac) & (rb + sd["len"] > ix.l_pac)).any()  # bridging seeds are dropped
                n_hi += int((rb > TWO32).any())
            n_chains += len(chains)
    assert n_chains > 500 and n_hi > 100, (n_chains, n_hi)
