"""tests/tinyindex.py -- the brute-force index of tiny and degenerate genomes the FM-index GPU tests run on -- and the
oracle on those indices: against the plain suffix sort on every row, and, where the compiled reference is present,
byte for byte against `bwa index` and call by call against the reference's bwt_sa / bwt_smem1 under every seeding
option set.  This is what makes the oracle the reference of tests/test_fmindex_tiny_gpu.py."""
import numpy as np
import pytest

import kswlib
import reflib
import tinyindex as ti

NEED_REF = pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built (no reference sources here)")
NAMES = list(ti.SHAPES)


def test_shapes_cover_the_index_edges():
    seq_lens, absent, primary_1, primary_last, primary_end = set(), False, False, False, False
    for name in NAMES:
        (primary, L2, n, words, sa_intv, samp), sa = ti.shape(name)
        assert n == 2 * len(ti.SHAPES[name]) and L2[0] == 0 and L2[4] == n and len(sa) == n + 1
        assert len(words) == (n + 15) // 16 + ((n + 127) // 128 + 1) * 8 and len(samp) == n // 32 + 1  # bwt_bwtupdate_core, bwt_cal_sa
        seq_lens.add(n)
        absent |= bool(ti.absent_bases(ti.shape(name)[0]))
        primary_1 |= primary == 1
        primary_end |= primary == n
        primary_last |= n > 128 and primary // 128 == (n - 1) // 128  # the sentinel's row in the last of several blocks
    assert seq_lens >= {16, 32, 126, 128, 200, 256, 300, 2000}
    assert absent and primary_1 and primary_last and primary_end
    assert ti.shape("homo_c64")[0][1] == [0, 0, 64, 128, 128]
    # the ten genomes the oracle was first checked on
    assert set(NAMES) >= {"homo_a16", "homo_c64", "ac_63", "at_64", "rand_8", "rand_64", "rand_100", "rand_128", "rand_1000", "acg_x50"}


def test_reads_hold_what_they_should():
    for name in NAMES:
        raw, _ = ti.shape(name)
        reads = ti.reads_for(name)
        assert 100 <= len(reads) <= 600
        assert sum(len(r) == 1 for r in reads) >= 5 and any((r == 4).any() for r in reads)
        for c in ti.absent_bases(raw):
            assert sum(len(r) > 1 and (r == c).all() for r in reads) >= 3
        if raw[2] <= 32:
            assert len(reads) >= raw[2] * (raw[2] + 1) // 2


@pytest.mark.parametrize("name", NAMES)
def test_oracle_sa_matches_plain_sort_on_every_row(name):
    raw, sa = ti.shape(name)
    cb = kswlib.make_cbwt(*raw, keep := [])
    assert (kswlib.orc_sa(cb, np.arange(raw[2] + 1)) == ti.sa_rows(sa)).all()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_intervals_are_the_rows_of_the_match(name):
    """Internal consistency without the reference: every interval the oracle returns is exactly the set of suffixes that
    start with the matched substring (counted by a plain scan of the text), under every option set."""
    raw, sa = ti.shape(name)
    cb = kswlib.make_cbwt(*raw, keep := [])
    text = bytes(ti.doubled(ti.SHAPES[name]))
    n_intv = 0
    for rd in ti.reads_for(name)[::4]:
        for oname in kswlib.SMEM_OPTION_SETS:
            calls, pool = kswlib.orc_smem_calls(cb, kswlib.smem_option_set(oname), rd)
            for v in pool:
                b, e = int(v["info"]) >> 32, int(v["info"]) & 0xffffffff
                sub = bytes(rd[b:e])
                occ = sorted(i for i in range(len(text) - len(sub) + 1) if text[i:i + len(sub)] == sub)
                x0, x2 = int(v["x0"]), int(v["x2"])
                assert sorted(sa[x0:x0 + x2]) == occ, (name, oname, b, e)
                n_intv += 1
    assert n_intv > 100


# ---- against the reference ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref_indices(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiny_index")
    out = {}
    for name in NAMES:
        fa = str(d / (name + ".fa"))
        reflib.write_fasta(fa, name, ti.SHAPES[name])
        reflib.build_index(fa)
        out[name] = reflib.lib().bwa_idx_load(fa.encode(), 7)
    yield out
    for idx in out.values():
        reflib.lib().bwa_idx_destroy(idx)


@pytest.mark.ref
@NEED_REF
@pytest.mark.parametrize("name", NAMES)
def test_tiny_index_is_byte_identical_to_bwa_index(ref_indices, name):
    (primary, L2, n, words, sa_intv, samp), sa = ti.shape(name)
    r_primary, r_L2, r_n, r_words, r_sa_intv, r_samp = reflib.bwt_arrays(ref_indices[name])
    assert (r_primary, r_L2, r_n, r_sa_intv) == (primary, L2, n, sa_intv)
    assert len(r_words) == len(words) and (r_words == words).all()
    assert len(r_samp) == len(samp) and (r_samp == samp).all()


@pytest.mark.ref
@NEED_REF
@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_tiny_indices(ref_indices, name):
    """bwt_sa on every row, and every bwt_smem1 call the oracle makes under every option set (start_width 2 and 3,
    split_len 0, split_width 0 and 1000 among them) with the same arguments through the reference."""
    raw, sa = ti.shape(name)
    idx = ref_indices[name]
    cb = kswlib.make_cbwt(*raw, keep := [])
    rows = np.arange(raw[2] + 1)
    want = reflib.ref_sa(idx, rows)
    assert (want == ti.sa_rows(sa)).all()
    assert (kswlib.orc_sa(cb, rows) == want).all()
    n_calls = 0
    for rd in ti.reads_for(name):
        for oname in kswlib.SMEM_OPTION_SETS:
            calls, pool = kswlib.orc_smem_calls(cb, kswlib.smem_option_set(oname), rd)
            n_calls += len(calls)
            for c in calls:
                ret, iv = reflib.ref_smem1(idx, rd, int(c["x"]), int(c["min_intv"]))
                mine = pool[int(c["first"]): int(c["first"]) + int(c["n"])]
                assert ret == int(c["ret"]) and len(iv) == len(mine) and (iv == mine).all(), (name, oname)
    assert n_calls > 1000
