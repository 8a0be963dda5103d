"""tests/redogen.py without a GPU: the slices that are to grow the overflow area of bmh_phase2_text_device's redo path do reach that
branch by the block's own arithmetic, before a GPU test trusts them with it.  Shorten redogen's long reads, or take some away, and
the inequalities here fail."""
import numpy as np
import pytest

import kswlib
import redogen as rg
import wantgen as wg


@pytest.fixture(scope="module")
def slices():
    whole, contigs = rg.growth_reference()
    return {name: (whole, contigs) + rg.growth(whole, spec) for name, spec in (("first", rg.FIRST), ("second", rg.SECOND))}


def test_the_bound_bounds_the_block():
    assert sum(rg.PER_REGION) == 668 and len(rg.PER_REGION) == 18
    for n, regions in ((1, 0), (1, 1), (48, 48), (130, 195), (32768, 70000), (7, 1), (63, 65)):
        assert 8 * (n + 1) + 128 + 668 * regions <= rg.lb_end(n, regions) <= rg.lb_max(n, regions), (n, regions)
    assert rg.first_cap(rg.lb_end(32768, 40000)) - rg.lb_end(32768, 40000) > 5 * rg.MIB  # (why a production slice never grows the block)


def test_md_len_gapless():
    assert rg.md_len_gapless(10, []) == 2                 # "10"
    assert rg.md_len_gapless(10, [0]) == 3                # "0A9"
    assert rg.md_len_gapless(10, [9]) == 3                # "9A0"
    assert rg.md_len_gapless(250, range(0, 250, 3)) == len("0A" + "2A" * 83 + "0")  # test_phase2_text_device_gpu.py::_outgrowing's long MD
    assert rg.md_len_gapless(2000, [5, 1500]) == len("5A1494A499")


@pytest.mark.parametrize("which", ["first", "second"])
def test_windows_and_md_lengths(slices, which):
    whole, contigs, reads, vectors, info = slices[which]
    half = contigs[1][0]
    assert len(reads) == len(vectors) == len(info["window"]) and len(info["md_len"]) == info["n_long"]
    n_short = 0
    for rd, v, win in zip(reads, vectors, info["window"]):
        a = v[0]
        assert len(v) == 1 and int(a["re"]) - int(a["rb"]) == win <= 65535 and (int(a["qb"]), int(a["qe"])) == (0, len(rd))
        lo = int(a["rb"]) if int(a["rb"]) < 2 * half else 4 * half - int(a["re"])  # on the forward strand
        assert lo // half == (lo + win - 1) // half  # inside one sequence: nothing for bwa_fix_xref2 to cut
        n_short += win == 150
    assert n_short >= 3 and all(m > rg.MD_SLOT for m in info["md_len"])
    # long and short reads alternate: no two ordinary reads, and never more than two long ones, next to each other
    kinds = "".join("s" if w == 150 else "L" for w in info["window"])
    assert "ss" not in kinds and "LLL" not in kinds and "LsL" in kinds


def test_the_first_slice_outgrows_a_fresh_block(slices):
    _, _, reads, vectors, info = slices["first"]
    bound = rg.first_cap(rg.lb_max(len(reads), sum(map(len, vectors))))
    predicted = rg.predicted_overflow(info)
    assert bound == rg.ceil_mib(1.25 * rg.lb_max(len(reads), sum(map(len, vectors)))) == rg.MIB
    assert predicted > bound and predicted >= 1.5 * bound, (predicted, bound)
    assert sum(info["md_len"]) > rg.MIB


def test_the_second_slice_outgrows_twice_what_the_first_leaves(slices):
    """ensure_keep asks for max(bytes, 2 * capacity): the first slice stays under twice the fresh block's capacity, the second passes
    twice the capacity the first leaves behind, so each branch of the maximum is taken once"""
    _, _, r1, v1, i1 = slices["first"]
    _, _, r2, v2, i2 = slices["second"]
    lb1 = rg.lb_max(len(r1), sum(map(len, v1)))
    cap0 = rg.first_cap(lb1)
    cap1, by_bytes = rg.grown_cap(cap0, lb1 + rg.predicted_overflow(i1) + 4 * 64)
    assert not by_bytes and cap1 == 3 * rg.MIB
    predicted = rg.predicted_overflow(i2)
    assert rg.lb_max(len(r2), sum(map(len, v2))) < cap1  # (the second slice's own block fits: only its overflow area makes it grow)
    assert predicted > 1.15 * 2 * cap1 and predicted > 2.5 * rg.predicted_overflow(i1), (predicted, cap1)
    assert rg.grown_cap(cap1, predicted)[1]


def test_the_oracle_aligns_the_long_reads_without_a_gap(slices):
    """mem_reg2aln's loop over bwa_gen_cigar2 (the CPU oracle) on one long read of each kind and strand: one match run, and an MD of the
    predicted length; the read without a DP in one try"""
    whole, contigs, reads, vectors, info = slices["first"]
    l_pac = len(whole)
    pac, p = wg.pack(whole), kswlib.make_params()
    longs = [(rd, v[0], m) for (rd, v, m) in zip([r for r, w in zip(reads, info["window"]) if w != 150],
                                                 [v for v, w in zip(vectors, info["window"]) if w != 150], info["md_len"])]
    seen = set()
    for rd, a, md_len in longs:
        key = (len(rd), int(a["rb"]) >= l_pac)
        if key in seen:
            continue
        seen.add(key)
        req = dict(qb=0, qe=len(rd), rb=int(a["rb"]), re=int(a["re"]), truesc=int(a["truesc"]), reg_w=int(a["w"]))
        score, words, nm, md, tries = kswlib.orc_reg2cigar(p, l_pac, pac, rd, req)
        assert list(words) == [len(rd) << 4] and len(md) == md_len and nm == len(np.arange(1, len(rd), 2 if len(rd) == rg.LONG else 3)), key
    assert seen == {(rg.LONG, False), (rg.LONG, True), (rg.ALIGNED, False), (rg.ALIGNED, True)}
