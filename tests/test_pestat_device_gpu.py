"""mem_pestat's pair walk on the device (pestat_collect_kernel, csrc/pestat.hip): bmh_pestat_device against the host's
bmh_pestat_candidates (the same text, host/pestat_core.h) word for word, on the reference's fixture groups and on the hand-made
vectors of tests/pestat_ref.py, at the 64-lane block edges; and behind bmh_chains2regs_device / bmh_seed_chain_regs_batch
(bmh_ctx_set_pestat_collect, bmh_ctx_set_regs_drop_exact): the regions are the switch-off call's (less the exact matches the host's
mem_test_and_remove_exact removes), the words are the host's on the returned vectors."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

import kswgen
import kswlib
import orientgen as og
import pestat_ref as pr
import postgen
import reflib
from __graft_entry__ import load_package
from test_chain2reg_gpu import _ctx, _same
from test_chain_gpu import _default_opt, _smem_opt
from test_pestat_cand_cpu import L_PAC, PAIR_KEYS, bits
from test_postproc_cpu import sam_opt, split
from test_region_dedup_gpu import _host_dedup

pytestmark = pytest.mark.gpu

ALNREG = kswlib.ALNREG


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # neither parameters nor a reference
    yield c
    c.close()


# ---------------------------------------------------------------- bmh_pestat_device against bmh_pestat_candidates

@pytest.mark.parametrize("key", PAIR_KEYS)
def test_orient_fixture_groups(pkg, ctx, key):
    _, si, _, l_pac, vecs, _, want_pes, _ = og.pairing_group(key)
    o = sam_opt(**postgen.OPTION_SETS[si])
    w = ctx.pestat_device(o, l_pac, vecs)
    assert (w == pkg.pestat_candidates(o, l_pac, vecs)).all() and (w != 0).sum() > 100
    assert bits(pkg.pestat_from_candidates(o, w)) == bits(want_pes)  # the reference's table


def test_postproc_fixture_pairs(pkg, ctx):
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "postproc_golden.npz"))
    for si, kw in enumerate(postgen.OPTION_SETS):
        p, o = f"s{si}_", sam_opt(**kw)
        vecs = split(g[p + "pairs"], g[p + "pairs_off"])
        w = ctx.pestat_device(o, 1_000_000, vecs)
        assert (w == pkg.pestat_candidates(o, 1_000_000, vecs)).all()
        assert bits(pkg.pestat_from_candidates(o, w)) == bits(g[p + "pes"])


@pytest.mark.parametrize("kw", [dict(), dict(max_ins=600, min_seed_len=25), dict(a=2, b=8, mask_level=0.25)])
def test_handmade_vectors(pkg, ctx, kw):
    o = sam_opt(**kw)
    vecs = pr.handmade(o, L_PAC)
    want, seen = pr.words(o, L_PAC, vecs)
    assert not [t for t in pr.ALL_TAGS if not seen.get(t)]
    assert {len(v) for v in vecs} >= {0, 1, 2, 40}
    w = ctx.pestat_device(o, L_PAC, vecs)
    assert (w == want).all(), np.nonzero(w != want)[0][:5]
    assert (w == pkg.pestat_candidates(o, L_PAC, vecs)).all()


@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65, 128, 129])
def test_block_edges(pkg, ctx, n_pairs):
    """The last pair is always a candidate with a distinctive size; vectors of 0, 1, 2 and 40 regions in between."""
    o = sam_opt()
    pool = pr.handmade(o, L_PAC)
    pool = pool[-16:] + pool[:-16]  # the 40-region vectors first
    vecs = [pool[k % len(pool)] for k in range(2 * max(n_pairs - 1, 0))] + (pr.pair_of(L_PAC, 2, 7777) if n_pairs else [])
    for odd_tail in ([], [pr.reg(5)]):  # an odd n ignores the last read
        w = ctx.pestat_device(o, L_PAC, vecs + odd_tail)
        assert len(w) == n_pairs and (w == pkg.pestat_candidates(o, L_PAC, vecs)).all()
        if n_pairs:
            assert w[-1] == (2 << 30 | 7777)
        if n_pairs >= 63:
            assert {len(v) for v in vecs} >= {0, 1, 2, 40} and (w != 0).sum() > 20


def test_empty_batches_and_bad_arguments(pkg, ctx):
    lib, o = pkg.lib(), sam_opt()
    assert len(ctx.pestat_device(o, L_PAC, [])) == 0
    w = ctx.pestat_device(o, L_PAC, [np.zeros(0, ALNREG)] * 140)
    assert len(w) == 70 and not w.any()
    v0 = pr.reg(1000)
    arr = (pkg._AlnregV * 2)()
    arr[0].n = arr[0].m = 1
    arr[0].a = v0.ctypes.data
    arr[1].n, arr[1].a = 3, None  # n > 0 and a == NULL
    out = np.full(1, 0xdead, dtype=np.uint32)
    op, ap, wp = o.ctypes.data_as(C.c_void_p), C.cast(arr, C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.bmh_pestat_device(ctx._h, op, L_PAC, 2, ap, wp) == pkg.BMH_E_ARG
    assert lib.bmh_pestat_device(ctx._h, op, L_PAC, -1, ap, wp) == pkg.BMH_E_ARG
    assert lib.bmh_pestat_device(ctx._h, op, L_PAC, 2, None, wp) == pkg.BMH_E_ARG
    assert lib.bmh_pestat_device(ctx._h, None, L_PAC, 2, ap, wp) == pkg.BMH_E_ARG
    assert lib.bmh_pestat_device(None, op, L_PAC, 2, ap, wp) == pkg.BMH_E_ARG
    arr[1].n, arr[1].a = 2 ** 31, v0.ctypes.data  # more than 2^31-1 regions in all; refused before anything is read
    assert lib.bmh_pestat_device(ctx._h, op, L_PAC, 2, ap, wp) == pkg.BMH_E_ARG
    arr[1].n = 1
    big = sam_opt(max_ins=1 << 30)
    assert lib.bmh_pestat_device(ctx._h, big.ctypes.data_as(C.c_void_p), L_PAC, 2, ap, wp) == pkg.BMH_E_RANGE
    assert out[0] == 0xdead
    assert lib.bmh_pestat_device(ctx._h, op, L_PAC, 0, None, None) == pkg.BMH_OK
    pair = pr.pair_of(L_PAC, 1, 300)
    assert ctx.pestat_device(o, L_PAC, pair)[0] == (1 << 30 | 300)  # the context serves the next call


# ---------------------------------------------------------------- behind the chains-to-regions calls

def _tandem_world():
    """test_chain2reg_gpu's world -- the repeat-rich genome of tools/make_chain_fixture.py, indexed by the compiled reference -- with
    40 tandem duplications of 25-40 bases planted.  A read that crosses one with a copy more or less than the genome has seeds that
    overlap on the read on two diagonals, which mem_chain2aln extends both (bwamem.c:787-794): redundant regions, the ones
    mem_sort_and_dedup removes.  (Without them one read in 300 loses a region.)"""
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_chain_fixture
    rng = np.random.default_rng(20262)
    ref, fams = make_chain_fixture.build(rng, 300_000)
    ref = np.asarray(ref, dtype=np.uint8)
    sites = []
    for j in range(40):
        P, s = int(rng.integers(25, 41)), 5000 + 7000 * j  # noqa: N806
        ref[s + P:s + 2 * P] = ref[s:s + P]
        sites.append((s, P))
    tmp = tempfile.mkdtemp(prefix="bmh_pestat_gpu_")
    fa = os.path.join(tmp, "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac, pac = reflib.pac_of(idx)
    return {"rng": rng, "ref": ref, "fams": fams, "sites": sites, "l_pac": l_pac, "pac": pac, "raw": reflib.bwt_arrays(idx), "idx": idx}


@pytest.fixture(scope="module")
def world():
    return _tandem_world()


def _pairs(world, n_pairs, L=100):  # noqa: N803
    """Read pairs (flat, 2 per pair) over that genome, in turn: a lightly mutated FR pair from anywhere; an error-free FR pair
    (truesc == l_seq * a: exact matches); mate 1 error-free from inside a repeat copy (an exact match with other copies' regions
    behind it) with a mutated mate; two mutated reads that hang over the edges of repeat copies; mate 1 across a tandem duplication
    with one copy or three where the genome has two (redundant regions)."""
    rng, ref, fams, sites = np.random.default_rng(515), world["ref"], world["fams"], world["sites"]
    rc = lambda s: (3 - s[::-1]).astype(np.uint8)  # noqa: E731
    long_fams = [f for f in fams if f[0][1] >= L + 40]
    out = []
    for k in range(n_pairs):
        kind, d = k % 5, int(rng.integers(250, 600))
        if kind in (2, 3):
            dst, Lf = long_fams[int(rng.integers(0, len(long_fams)))][int(rng.integers(0, 6))]
            pos = dst + (int(rng.integers(0, Lf - L)) if kind == 2 else int(rng.integers(-L // 2, Lf - L // 2)))
        else:
            pos = int(rng.integers(1000, len(ref) - 2000))
        pos = min(max(pos, 700), len(ref) - 1000)
        rate = 0.0 if kind in (1, 2) else 0.05 if kind == 3 else float(rng.choice([0.01, 0.03]))
        L1 = int(rng.integers(150, 251)) if kind == 3 else L  # noqa: N806
        m1 = kswgen.mutate(rng, ref[pos:pos + L1 + 20], rate, 0.003 if rate else 0.0, 0.003 if rate else 0.0, 3)[:L1].copy()
        rate2 = 0.0 if kind == 1 else 0.05 if kind == 3 else 0.02
        m2 = rc(kswgen.mutate(rng, ref[pos + d - L1 - 20:pos + d], rate2, 0.0, 0.0, 3)[-L1:].copy())
        if kind == 3 and k % 3 == 0:
            at = int(rng.integers(0, L1))
            m1[at:at + int(rng.integers(1, 10))] = 4
        if kind == 4:
            s, P = sites[int(rng.integers(0, len(sites)))]  # noqa: N806
            m1 = np.concatenate([ref[s - 50:s]] + [ref[s:s + P]] * (1 if k % 2 else 3) + [ref[s + 2 * P:s + 2 * P + 50]])
            m2 = rc(ref[s + d - L:s + d].copy())
        pair = [m1, m2]
        if k % 8 >= 4:  # the pair on the other strand
            pair = [m2, m1]
        out += [np.ascontiguousarray(r, dtype=np.uint8) for r in pair]
    return out


def test_collect_and_drop_exact_behind_the_region_calls(pkg, world):  # noqa: F811
    p = kswlib.make_params()
    o = _default_opt()
    so = _smem_opt(o)
    sopt = sam_opt()
    l_pac, match = world["l_pac"], int(p["a"])
    ctx = _ctx(world, p)
    with pytest.raises(pkg.BmhError) as e:  # before any collecting call
        ctx.last_pestat_candidates(0)
    assert e.value.code == pkg.BMH_E_ARG and ctx.last_drop_exact_stats() == -1
    reads = _pairs(world, 240)
    n, lens = len(reads), [len(r) for r in reads]
    msl = int(o["min_seed_len"])
    chains = ctx.seed_chain_batch(so, o, l_pac, reads)
    for name, call in (("chains2regs_device", lambda: ctx.chains2regs_device(l_pac, reads, chains, msl)),
                       ("seed_chain_regs_batch", lambda: ctx.seed_chain_regs_batch(so, o, l_pac, reads, msl))):
        ctx.set_pestat_collect(False), ctx.set_regs_drop_exact(False), ctx.set_regs_dedup(False, 0.95)
        raw = call()
        want = [_host_dedup(a, 0.95) for a in raw]
        # de-duplication removed regions from some reads: a kernel that read the slice lengths in place of the counts would show here
        assert sum(len(a) > len(b) for a, b in zip(raw, want)) >= 5, name
        ctx.set_regs_dedup(True, 0.95)
        base = call()
        _same(base, want, f"{name}, de-duplication only")
        s_base, d_base = ctx.driver_stats(), ctx.last_dedup_stats()[:2]
        # collect
        ctx.set_pestat_collect(True, sopt)
        got = call()
        _same(got, base, f"{name}, collect on")
        w, ms = ctx.last_pestat_candidates(n // 2)
        host_w = pkg.pestat_candidates(sopt, l_pac, got)
        assert (w == host_w).all(), (name, np.nonzero(w != host_w)[0][:5])
        assert (w != 0).sum() >= 50 and ms == -1.0, (name, (w != 0).sum(), ms)
        assert ctx.driver_stats() == s_base and ctx.last_dedup_stats()[:2] == d_base
        with pytest.raises(pkg.BmhError) as e:
            ctx.last_pestat_candidates(n // 2 + 1)
        assert e.value.code == pkg.BMH_E_ARG
        # drop-exact with collect: the host's mem_test_and_remove_exact on the switch-off vectors, and the words of what is left
        exact = [len(a) > 0 and int(a[0]["truesc"]) == lens[r] * match for r, a in enumerate(base)]
        assert sum(exact) >= 20, (name, sum(exact))
        assert sum(e_ and len(a) == 1 for e_, a in zip(exact, base)) >= 5 and sum(e_ and len(a) > 1 for e_, a in zip(exact, base)) >= 5, name
        want2, gone = pr.drop_exact(base, lens, match)
        ctx.set_regs_drop_exact(True)
        got2 = call()
        _same(got2, want2, f"{name}, drop-exact on")
        w2, _ = ctx.last_pestat_candidates(n // 2)
        assert (w2 == pkg.pestat_candidates(sopt, l_pac, want2)).all() and (w2 != w).any(), name
        assert ctx.last_drop_exact_stats() == gone == sum(exact)
        assert ctx.driver_stats() == s_base and ctx.last_dedup_stats()[:2] == d_base  # they report what they report without the switches
        # drop-exact alone
        ctx.set_pestat_collect(False)
        _same(call(), want2, f"{name}, drop-exact alone")
        assert ctx.last_drop_exact_stats() == gone
        with pytest.raises(pkg.BmhError) as e:
            ctx.last_pestat_candidates(n // 2)
        assert e.value.code == pkg.BMH_E_ARG
    # drop-exact alone on an odd batch: the lone last read is served too
    odd = 2 * next(k for k in range(n // 2) if exact[2 * k]) + 1
    _same(ctx.chains2regs_device(l_pac, reads[:odd], chains[:odd], msl), want2[:odd], "drop-exact alone, odd batch")
    ctx.close()


def test_refusals_leave_the_switches_and_the_context(pkg, world):  # noqa: F811
    p = kswlib.make_params()
    o = _default_opt()
    so = _smem_opt(o)
    sopt = sam_opt()
    l_pac, msl = world["l_pac"], int(o["min_seed_len"])
    ctx = _ctx(world, p)
    reads = _pairs(world, 40)
    chains = ctx.seed_chain_batch(so, o, l_pac, reads)
    ctx.set_regs_dedup(True, 0.95)
    ctx.set_pestat_collect(True, sopt)
    good = ctx.chains2regs_device(l_pac, reads, chains, msl)
    w_good, _ = ctx.last_pestat_candidates(len(reads) // 2)

    def refused(code, call, needle=None):
        with pytest.raises(pkg.BmhError) as e:
            call()
        assert e.value.code == code and (needle is None or needle in str(e.value)), e.value

    def serves():
        _same(ctx.chains2regs_device(l_pac, reads, chains, msl), good, "after a refusal")
        assert (ctx.last_pestat_candidates(len(reads) // 2)[0] == w_good).all()

    # an odd n_reads with collect on
    refused(pkg.BMH_E_ARG, lambda: ctx.chains2regs_device(l_pac, reads[:7], chains[:7], msl))
    refused(pkg.BMH_E_ARG, lambda: ctx.seed_chain_regs_batch(so, o, l_pac, reads[:7], msl))
    serves()
    # either switch with regs_dedup off; the message names the switch
    ctx.set_regs_dedup(False, 0.95)
    refused(pkg.BMH_E_ARG, lambda: ctx.chains2regs_device(l_pac, reads, chains, msl), "bmh_ctx_set_pestat_collect")
    ctx.set_pestat_collect(False), ctx.set_regs_drop_exact(True)
    refused(pkg.BMH_E_ARG, lambda: ctx.seed_chain_regs_batch(so, o, l_pac, reads, msl), "bmh_ctx_set_regs_drop_exact")
    ctx.set_regs_drop_exact(False), ctx.set_pestat_collect(True, sopt), ctx.set_regs_dedup(True, 0.95)
    serves()
    # max_ins = 2^30
    ctx.set_pestat_collect(True, sam_opt(max_ins=1 << 30))
    refused(pkg.BMH_E_RANGE, lambda: ctx.chains2regs_device(l_pac, reads, chains, msl))
    ctx.set_pestat_collect(True, sopt)
    serves()
    # a wrong pair count
    refused(pkg.BMH_E_ARG, lambda: ctx.last_pestat_candidates(len(reads) // 2 - 1))
    serves()
    # a successful call without reads is a collecting call of 0 pairs: the earlier call's words are not served for it
    assert ctx.chains2regs_device(l_pac, [], [], msl) == []
    w0, ms0 = ctx.last_pestat_candidates(0)
    assert len(w0) == 0 and ms0 == -1.0
    refused(pkg.BMH_E_ARG, lambda: ctx.last_pestat_candidates(len(reads) // 2))
    serves()
    # timing mode: the kernel's duration, and -1 without
    assert ctx.last_pestat_candidates(len(reads) // 2)[1] == -1.0
    ctx.set_kernel_timing(True)
    _same(ctx.chains2regs_device(l_pac, reads, chains, msl), good, "timing mode")
    w, ms = ctx.last_pestat_candidates(len(reads) // 2)
    assert (w == w_good).all() and ms >= 0.0
    ctx.set_kernel_timing(False)
    ctx.close()
