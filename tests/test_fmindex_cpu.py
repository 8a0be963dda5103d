"""FM-index queries of the seeding stage: the CPU restatement oracle/fmindex_oracle.c against
the committed fixture (outputs of the reference's bwt_smem1 / bwt_sa on an index the reference built) and, where the
compiled reference is present, against the reference's functions live -- including smem_next2's merged output, which
pins the ORDER of bwt_smem1 calls the restatement makes."""
import numpy as np
import pytest

import kswlib
import reflib


def _same_calls(got, want):
    (gc, gi), (wc, wi) = got, want
    return len(gc) == len(wc) and all((gc[f] == wc[f]).all() for f in ("x", "min_intv", "ret", "n", "first")) and \
        len(gi) == len(wi) and (gi == wi).all()


def test_oracle_fmindex_matches_reference_fixture():
    cb, keep, raw, opt, reads, per, sa_k, sa_pos = kswlib.golden_fmindex()
    assert len(reads) >= 400 and sum(len(c) for c, _ in per) > 4000
    for rd, want in zip(reads, per):
        assert _same_calls(kswlib.orc_smem_calls(cb, opt, rd), want)
    assert (kswlib.orc_sa(cb, sa_k) == sa_pos).all()


def _orc_calls(cb, opt, rd):
    """orc_smem_calls, with an empty read giving no calls."""
    return kswlib.orc_smem_calls(cb, opt, rd) if len(rd) else (np.zeros(0, kswlib.SMEM_CALL), np.zeros(0, kswlib.SMEM_INTV))


def _intv_len(iv):
    return (iv["info"] & np.uint64(0xffffffff)).astype(np.int64) - (iv["info"] >> np.uint64(32)).astype(np.int64)


def _reseeding(calls, opt):
    """Calls that cannot be main calls: their min_intv is not start_width.  A lower bound on the re-seeding calls (one whose
    longest match occurs start_width - 1 times has min_intv == start_width)."""
    return int((calls["min_intv"] != int(opt["start_width"])).sum())


def fixture_reads(seed, n, lengths, muts):
    """n reads cut from the fixture's own reads (they come from the indexed genome) and re-mutated: each with a length of
    `lengths` and a per-base mutation rate of `muts`; a mutated base becomes another base or N."""
    cb, keep, raw, opt, reads, per, sa_k, sa_pos = kswlib.golden_fmindex()
    rng = np.random.default_rng(seed)
    src = np.concatenate(reads)
    out = []
    for _ in range(n):
        L = int(rng.choice(lengths))
        p = int(rng.integers(0, len(src) - L))
        rd = src[p:p + L].copy()
        m = rng.random(L) < float(rng.choice(muts))
        rd[m] = (rd[m] + rng.integers(1, 4, int(m.sum()))) % 5
        out.append(rd)
    return out


_matrix = {}


def option_matrix_reads_and_oracle():
    """The 1 500 reads of the option matrix and the oracle's answer for every (set, emit), computed once per process."""
    if not _matrix:
        cb, keep, raw, opt, reads, per, sa_k, sa_pos = kswlib.golden_fmindex()
        more = fixture_reads(211, 1500, [1, 18, 19, 20, 75, 150, 151, 300], [0.0, 0.02, 0.12])
        want = {(oname, emit): [_orc_calls(cb, kswlib.smem_option_set(oname, emit), rd) for rd in more]
                for oname in kswlib.SMEM_OPTION_SETS for emit in (False, True)}
        _matrix["v"] = (more, want)
    return _matrix["v"]


def test_option_sets_differ_on_the_oracle():
    """The option matrix is only a matrix if its sets lead to different work: counted on the ORACLE's output for the 1 500
    reads (on 600 reads of this recipe it gave 5 645 calls / 406 re-seeding calls for `fixture`, 7 652 calls for
    `no_exact`, 7 737 for `short`, 5 239 / 0 for `split_off` and `width0`, 6 710 / 1 471 for `eager`, 8 391 for `sw3`)."""
    more, want = option_matrix_reads_and_oracle()
    n_calls, n_re = {}, {}
    for oname in kswlib.SMEM_OPTION_SETS:
        o = kswlib.smem_option_set(oname)
        n_calls[oname] = sum(len(c) for c, _ in want[oname, False])
        n_re[oname] = sum(_reseeding(c, o) for c, _ in want[oname, False])
        # min_emit_len never changes the calls
        assert all(len(c) == len(e) and (c["x"] == e["x"]).all() and (c["min_intv"] == e["min_intv"]).all()
                   for (c, _), (e, _) in zip(want[oname, False], want[oname, True]))
    assert n_re["split_off"] == 0 and n_re["width0"] == 0
    assert all(_same_calls(a, b) for a, b in zip(want["split_off", False], want["width0", False]))
    assert n_re["eager"] >= 1500 and n_re["fixture"] >= 400
    for oname in ("no_exact", "short", "sw3"):
        assert n_calls[oname] >= 1.2 * n_calls["fixture"], (oname, n_calls)


@pytest.fixture(scope="module")
def live_index(tmp_path_factory):
    import kswgen
    rng = np.random.default_rng(181)
    ref = kswgen.rand_seq(rng, 50000)
    for _ in range(15):
        a, b, L = int(rng.integers(0, 47000)), int(rng.integers(0, 47000)), int(rng.integers(80, 400))
        ref[b:b + L] = kswgen.mutate(rng, ref[a:a + L + 20], 0.01, 0.002, 0.002, 2)[:L]
    fa = str(tmp_path_factory.mktemp("live_index") / "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    prim, L2, sl, words, sai, sa = reflib.bwt_arrays(idx)
    keep = []
    cb = kswlib.make_cbwt(prim, L2, sl, words, sai, sa, keep)
    reads = []
    for it in range(150):
        Lr = int(rng.integers(30, 250))
        pos = int(rng.integers(0, len(ref) - Lr - 12))
        rd = kswgen.mutate(rng, ref[pos:pos + Lr + 10], 0.03, 0.004, 0.004, 3)[:Lr].copy()
        if it % 3 == 0:
            rd[rng.random(len(rd)) < 0.03] = 4
        reads.append(rd)
    ks = rng.integers(0, sl + 1, 2000).astype(np.uint64)
    yield idx, cb, keep, sl, reads, ks
    reflib.lib().bwa_idx_destroy(idx)


@pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built (no /root/reference here)")
@pytest.mark.parametrize("oname", list(kswlib.SMEM_OPTION_SETS))
def test_oracle_fmindex_matches_reference_live(live_index, oname):
    """Every option set of kswlib.SMEM_OPTION_SETS through the reference: each call the oracle makes == bwt_smem1 with the
    same arguments, and -- where mem_opt_t can express the set (start_width 1, or 2 through MEM_F_NO_EXACT) -- the calls
    are the ones smem_next2 makes.  With min_emit_len = min_seed_len: the same calls, the long intervals only."""
    idx, cb, keep, sl, reads, ks = live_index
    msl, split_len, split_width, start_width = kswlib.SMEM_OPTION_SETS[oname]
    so = kswlib.smem_option_set(oname)
    so_emit = kswlib.smem_option_set(oname, emit=True)
    opt = None
    if start_width <= 2:  # mem_opt_t as `bwa mem` would fill it; smem_opt_of reads our four numbers back out of it
        opt = reflib.opt_from_params(kswlib.make_params())
        opt.contents.min_seed_len, opt.contents.split_width = msl, split_width
        opt.contents.split_factor = split_len / msl
        opt.contents.flag = (opt.contents.flag & ~0x40) | (0x40 if start_width == 2 else 0)  # MEM_F_NO_EXACT
        back = reflib.smem_opt_of(opt)
        assert all(int(back[f]) == int(so[f]) for f in ("min_seed_len", "split_len", "split_width", "start_width"))
    if oname == "fixture":
        assert (kswlib.orc_sa(cb, ks) == reflib.ref_sa(idx, ks)).all()
    n_calls = 0
    for rd in reads:
        calls, pool = kswlib.orc_smem_calls(cb, so, rd)
        ecalls, epool = kswlib.orc_smem_calls(cb, so_emit, rd)
        assert len(ecalls) == len(calls)
        n_calls += len(calls)
        for c, e in zip(calls, ecalls):  # every call == the reference's bwt_smem1 with the same arguments
            ret, iv = reflib.ref_smem1(idx, rd, int(c["x"]), int(c["min_intv"]))
            mine = pool[int(c["first"]): int(c["first"]) + int(c["n"])]
            assert ret == int(c["ret"]) and len(iv) == len(mine) and (iv == mine).all()
            long_ = iv[_intv_len(iv) >= msl]
            assert all(int(c[k]) == int(e[k]) for k in ("x", "min_intv", "ret")) and int(e["n"]) == len(long_)
            assert (epool[int(e["first"]): int(e["first"]) + int(e["n"])] == long_).all()
        if opt is None:
            continue
        # ... and the calls are the ones smem_next2 makes: every interval it returns is one of ours, every main call's
        # return value is where its next iteration starts
        its = reflib.ref_smem_iter(idx, opt, rd)
        mains, at = [], 0  # a main call starts where the one before it returned (after any N), a re-seeding call inside that match
        for c in calls:
            while at < len(rd) and rd[at] > 3:
                at += 1
            if int(c["x"]) == at and int(c["min_intv"]) == start_width:
                mains.append(c)
                at = int(c["ret"])
        assert len(mains) == len(its)
        key = lambda w: tuple(int(w[f]) for f in ("x0", "x1", "x2", "info"))
        have = {key(v) for v in pool}
        for c, v in zip(mains, its):  # an iteration returns its main call's intervals and some of its re-seeding call's
            got = [key(w) for w in v]
            assert all(g in have for g in got)
            assert all(key(w) in got for w in pool[int(c["first"]): int(c["first"]) + int(c["n"])])
    assert n_calls > 1000


def test_oracle_min_emit_len_is_a_pure_filter():
    """bmh_smem_opt_t.min_emit_len hands back the long intervals of the same calls, in the same order."""
    cb, keep, raw, opt, reads, per, sa_k, sa_pos = kswlib.golden_fmindex()
    o2 = np.array(opt, dtype=kswlib.SMEM_OPT).copy()
    o2["min_emit_len"] = int(o2["min_seed_len"])
    n_short = 0
    for rd in reads:
        calls, pool = kswlib.orc_smem_calls(cb, opt, rd)
        fc, fp = kswlib.orc_smem_calls(cb, o2, rd)
        assert len(fc) == len(calls)
        want = []
        for c, f in zip(calls, fc):
            assert all(int(c[k]) == int(f[k]) for k in ("x", "min_intv", "ret"))
            iv = pool[int(c["first"]): int(c["first"]) + int(c["n"])]
            ln = (iv["info"] & np.uint64(0xffffffff)).astype(np.int64) - (iv["info"] >> np.uint64(32)).astype(np.int64)
            long_ = iv[ln >= int(o2["min_emit_len"])]
            n_short += len(iv) - len(long_)
            assert int(f["n"]) == len(long_) and (fp[int(f["first"]): int(f["first"]) + int(f["n"])] == long_).all()
            want.append(long_)
        assert len(fp) == sum(len(w) for w in want)
    assert n_short > 100
