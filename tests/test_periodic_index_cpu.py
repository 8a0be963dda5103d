"""tests/periodic_index.py -- the exact FM-index of a periodic genome the large-index GPU tests run on -- against a plain
suffix sort (tiny shapes), against `bwa index` itself (small shapes, compiled reference), and, on the hg38-sized index,
the oracle against the reference's bwt_smem1 / smem_next2 / bwt_sa and bmh_index_load against the generator."""
import ctypes as C
import os

import numpy as np
import pytest

import kswlib
import periodic_index as pi
import reflib
import tinyindex

NEED_REF = pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built (no reference sources here)")


def _brute(P, m):
    """Suffix array, BWT rows and bwa's arrays of P^(2m)$ from tests/tinyindex.py's plain suffix sort: P is its own reverse
    complement, so P^(2m) is the doubled text of the forward genome P^m."""
    assert (np.asarray(P) == 3 - np.asarray(P)[::-1]).all()
    (primary, L2, n, words, sa_intv, samp), sa = tinyindex.build(np.tile(P, m))
    assert n == 2 * m * len(P) and sa_intv == 32
    return sa, primary, L2, words, samp


@pytest.mark.parametrize("chunk", [1, 3, 1 << 18])
def test_generator_matches_brute_force(chunk):
    rng = np.random.default_rng(11 + chunk)
    n_shapes = 0
    for half in (2, 3, 5, 8, 13, 33, 70):
        for m in (1, 2, 3, 7, 16):
            if half * 2 * 2 * m > 9000:
                continue
            P = pi.make_period(rng, half, lead_t=int(rng.integers(0, 4)))
            ix = pi.PeriodicIndex(P, m, chunk_blocks=chunk, threads=2)
            sa, primary, L2, words, samp = _brute(P, m)
            n = len(sa) - 1
            assert ix.seq_len == n and ix.primary == primary and ix.L2 == L2, (half, m)
            assert ix.bwt_size == len(words) and (ix.bwt == words).all(), (half, m)
            assert ix.n_sa == len(samp) and (ix.sa == samp).all(), (half, m)
            assert (ix.sa_of(np.arange(n + 1)) == np.array([pi.U64_MAX] + sa[1:], np.uint64)).all(), (half, m)
            assert (ix.row_of(np.array(sa[1:])) == np.arange(1, n + 1)).all(), (half, m)
            n_shapes += 1
    assert n_shapes >= 25


def test_generator_covers_lengths_off_the_block_grid():
    """seq_len = 4*half*m: shapes where it is not a multiple of 128 (partial last block, partial last word) or of 32."""
    rng = np.random.default_rng(3)
    seen = set()
    for half, m in ((3, 1), (5, 3), (9, 5), (17, 2), (33, 3), (7, 9), (40, 2), (64, 1)):
        P = pi.make_period(rng, half)
        ix = pi.PeriodicIndex(P, m, chunk_blocks=2, threads=3)
        sa, primary, L2, words, samp = _brute(P, m)
        assert ix.primary == primary and ix.L2 == L2 and (ix.bwt == words).all() and (ix.sa == samp).all()
        seen.add((ix.seq_len % 128 == 0, ix.seq_len % 32 == 0, ix.seq_len % 16 == 0))
    assert (False, False, False) in seen and (False, True, True) in seen and (True, True, True) in seen


def test_suffix_array_pp_matches_plain_sort():
    rng = np.random.default_rng(5)
    for half in (1, 2, 4, 9, 31, 200, 1500):
        P = pi.make_period(rng, half, lead_t=0)
        S = bytes(np.concatenate([P, P]) + 1) + b"\0"
        want = sorted(range(len(S)), key=lambda i: S[i:])
        assert pi.suffix_array_pp(P).tolist() == want, half


def test_closed_form_occurrences():
    rng = np.random.default_rng(9)
    P = pi.make_period(rng, 50)
    ix = pi.PeriodicIndex(P, 3, threads=1)
    T = np.tile(P, 2 * 3)
    for r0, L in ((0, 30), (7, 100), (99, 40), (55, 150), (3, 590)):
        q = ix.substring(r0, L)
        want = [i for i in range(len(T) - L + 1) if np.array_equal(T[i:i + L], q)]
        assert ix.occurrences(r0, L).tolist() == want


# ---- against `bwa index` -------------------------------------------------------------------------------------------------

@pytest.mark.ref
@NEED_REF
@pytest.mark.parametrize("half,m", [(1000, 1), (1031, 3), (5000, 7), (20_011, 2), (2_000, 40), (100_000, 1), (100_003, 5)])
def test_generator_is_byte_identical_to_bwa_index(tmp_path, half, m):
    """The arrays bwa_idx_load hands out and the .pac `bwa index` writes, byte for byte: layout, primary, L2, SA sampling."""
    rng = np.random.default_rng(half * 7 + m)
    P = pi.make_period(rng, half)
    ix = pi.PeriodicIndex(P, m, chunk_blocks=97)
    fa = str(tmp_path / "per.fa")
    reflib.write_fasta(fa, "per", np.tile(P, m))
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    primary, L2, seq_len, words, sa_intv, sa = reflib.bwt_arrays(idx)
    assert (primary, L2, seq_len, sa_intv) == (ix.primary, ix.L2, ix.seq_len, ix.sa_intv)
    assert len(words) == ix.bwt_size and (words == ix.bwt).all()
    assert len(sa) == ix.n_sa and (sa == ix.sa).all()
    with open(fa + ".pac", "rb") as f:
        assert f.read() == ix.pac_bytes().tobytes()
    ks = rng.integers(0, seq_len + 1, 3000)
    assert (reflib.ref_sa(idx, ks) == ix.sa_of(ks)).all()
    reflib.lib().bwa_idx_destroy(idx)


# ---- the hg38-sized index ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_files(tmp_path_factory):
    ix = pi.big()
    prefix = str(tmp_path_factory.mktemp("periodic_big") / "per")
    ix.write_files(prefix)
    yield ix, prefix
    for ext in (".bwt", ".sa", ".pac", ".ann", ".amb"):
        os.remove(prefix + ext)


def _reads(rng, ix, n):
    out = []
    for k in range(n):
        L = int(rng.choice([19, 20, 36, 150, 151, 300]))
        if k % 5 == 4:
            out.append(rng.integers(0, 4, L).astype(np.uint8))  # random: small intervals
            continue
        r0 = int(rng.integers(0, ix.p)) if k % 5 else ix.p - int(rng.integers(1, L))  # or across the period seam
        rd = ix.substring(r0, L)
        m = rng.random(L) < float(rng.choice([0.0, 0.02, 0.12]))
        rd[m] = (rd[m] + rng.integers(1, 4, m.sum())) % 4
        if k % 7 == 0:
            rd[int(rng.integers(0, L)):][:int(rng.integers(1, 6))] = 4
        out.append(rd)
    return out


@pytest.mark.ref
@NEED_REF
def test_oracle_matches_reference_on_the_big_index(big_files):
    """bwt_smem1 / smem_next2 / bwt_sa of the reference, loaded from the generator's files, against oracle/fmindex_oracle.c
    at 6.2e9 rows: what makes the oracle the reference of the large GPU tests."""
    ix, prefix = big_files
    idx = reflib.lib().bwa_idx_load(prefix.encode(), 7)
    try:
        b = C.cast(idx.contents.bwt, C.POINTER(reflib.BwtT)).contents
        assert (b.primary, list(b.L2), b.seq_len) == (ix.primary, ix.L2, ix.seq_len)
        keep = []
        cb = kswlib.make_cbwt(*ix.raw(), keep)
        opt = reflib.opt_from_params(kswlib.make_params())
        so = reflib.smem_opt_of(opt)
        rng = np.random.default_rng(77)
        ks = np.concatenate([rng.integers(0, ix.seq_len + 1, 3000),
                             [0, 1, ix.primary - 1, ix.primary, ix.primary + 1, ix.seq_len - 1, ix.seq_len,
                              (1 << 32) - 1, 1 << 32, (1 << 32) + 1]]).astype(np.uint64)
        want = reflib.ref_sa(idx, ks)
        assert (kswlib.orc_sa(cb, ks) == want).all()
        assert (ix.sa_of(ks) == want).all()
        n_calls, hi = 0, 0
        for rd in _reads(rng, ix, 300):
            calls, pool = kswlib.orc_smem_calls(cb, so, rd)
            n_calls += len(calls)
            hi += int((pool["x0"] > np.uint64(1 << 32)).sum())
            for c in calls:
                ret, iv = reflib.ref_smem1(idx, rd, int(c["x"]), int(c["min_intv"]))
                mine = pool[int(c["first"]): int(c["first"]) + int(c["n"])]
                assert ret == int(c["ret"]) and len(iv) == len(mine) and (iv == mine).all()
            its = reflib.ref_smem_iter(idx, opt, rd)
            assert len([c for c in calls if int(c["min_intv"]) == int(so["start_width"])]) == len(its)
            have = {tuple(int(v[f]) for f in ("x0", "x1", "x2", "info")) for v in pool}
            assert all(tuple(int(w[f]) for f in ("x0", "x1", "x2", "info")) in have for v in its for w in v)
        assert n_calls > 300 and hi > 100
    finally:
        reflib.lib().bwa_idx_destroy(idx)


def test_index_load_round_trip_on_the_big_index(big_files):
    """bmh_index_load of the generator's 3.1 GB .bwt, 1.55 GB .sa and 16-contig .ann: offsets past 2^31."""
    from test_index_io import CIndex
    from __graft_entry__ import load_package
    ix, prefix = big_files
    L = load_package().lib()
    L.bmh_index_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(CIndex))]
    L.bmh_index_free.argtypes = [C.POINTER(CIndex)]
    px = C.POINTER(CIndex)()
    assert L.bmh_index_load(prefix.encode(), C.byref(px)) == 0
    try:
        x = px.contents
        b = x.bwt
        assert (b.primary, list(b.L2), b.seq_len, b.bwt_size, b.sa_intv, b.n_sa) == \
            (ix.primary, ix.L2, ix.seq_len, ix.bwt_size, ix.sa_intv, ix.n_sa)
        assert (np.ctypeslib.as_array(C.cast(b.bwt, C.POINTER(C.c_uint32)), (b.bwt_size,)) == ix.bwt).all()
        assert (np.ctypeslib.as_array(C.cast(b.sa, C.POINTER(C.c_uint64)), (b.n_sa,)) == ix.sa).all()
        assert x.l_pac == ix.l_pac and x.n_seqs == len(ix.contigs) == 16 and x.n_holes == 0
        got = [(x.names[k].decode(), x.offsets[k], x.lens[k]) for k in range(x.n_seqs)]
        assert got == ix.contigs and got[-1][1] > 1 << 31
        pac = ix.pac_bytes()
        assert (np.ctypeslib.as_array(C.cast(x.pac, C.POINTER(C.c_uint8)), (ix.l_pac // 4 + 1,)) == pac[:ix.l_pac // 4 + 1]).all()
    finally:
        L.bmh_index_free(px)
