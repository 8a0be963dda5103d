"""tests/golden/pipeline_golden.npz (tools/make_pipeline_fixture.py) is consistent with itself -- contig table, index arrays, SAM
bodies and the read shapes the reference's output is to contain, counted again here from the SAM text -- and, where oracle/_ref is
built, is what the compiled reference's `bwa mem` gives for its genome and reads today."""
import os
import sys

import numpy as np
import pytest

import kswlib
import pipechain as pc
import reflib

sys.path.insert(0, os.path.join(kswlib.ROOT, "tools"))
import make_pipeline_fixture as mk  # noqa: E402


def test_contig_table_and_packed_reference():
    w, g = pc.world(), pc.fixture()
    at = 0
    for (off, ln), name in zip(w.contigs, w.names):
        assert off == at and ln > 0 and name
        at += ln
    assert at == w.l_pac == len(w.genome) and len(set(w.names)) == len(w.names) == 3 and len({ln for _, ln in w.contigs}) == 3
    assert 40_000 <= w.l_pac <= 56_000 and int(w.genome.max()) <= 3
    pad = np.concatenate([w.genome, np.zeros(-w.l_pac % 4, np.uint8)]).reshape(-1, 4)
    packed = (pad[:, 0] << 6 | pad[:, 1] << 4 | pad[:, 2] << 2 | pad[:, 3]).astype(np.uint8)
    assert np.array_equal(w.pac[:len(packed)], packed)
    assert [str(x) for x in g["runs"]] == list(pc.RUNS)


def test_index_arrays_give_the_genomes_suffixes():
    """bwt_sa through the CPU oracle on a few hundred rows, sampled and not: each row's suffix of genome + reverse complement is not
    below the row before it (tests/tinyindex.py's check, on rows in place of a whole table), and the rows of the samples are a
    permutation's"""
    w = pc.world()
    prim, L2, seq_len, words, sa_intv, sa = w.raw  # noqa: N806
    both = np.concatenate([w.genome, (3 - w.genome[::-1]).astype(np.uint8)])
    assert seq_len == 2 * w.l_pac == len(both) and L2[4] == seq_len and L2[0] == 0
    assert [L2[k + 1] - L2[k] for k in range(4)] == [int((both == k).sum()) for k in range(4)]
    keep = []
    cb = kswlib.make_cbwt(prim, L2, seq_len, words, sa_intv, sa, keep)
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([[1, 2, seq_len - 1, seq_len], rng.integers(1, seq_len + 1, 300), rng.integers(1, seq_len // sa_intv, 50) * sa_intv]))
    ks = np.sort(np.unique(np.concatenate([rows, np.maximum(rows - 1, 1)]))).astype(np.uint64)
    pos = kswlib.orc_sa(cb, ks)
    assert len(set(pos.tolist())) == len(pos) and int(pos.max()) < seq_len
    for (k0, p0), (k1, p1) in zip(zip(ks[:-1], pos[:-1]), zip(ks[1:], pos[1:])):
        a, b = both[int(p0):], both[int(p1):]
        m = min(len(a), len(b))
        d = np.flatnonzero(a[:m] != b[:m])
        assert (a[d[0]] < b[d[0]]) if len(d) else len(a) <= len(b), (int(k0), int(k1))
    for k, p in zip(ks, pos):  # rows of a base: the suffix starts with it
        assert L2[both[int(p)]] < int(k) <= L2[both[int(p)] + 1], int(k)


@pytest.mark.parametrize("name", pc.RUNS)
def test_sam_body_and_options(name):
    r, g = pc.run(name), pc.fixture()
    n = len(r.reads)
    assert 180 <= n <= 420 and len(r.names) == n and len(r.sam_off) == n + 1
    assert r.sam_off[0] == 0 and r.sam_off[-1] == len(r.sam) and (np.diff(r.sam_off) > 0).all()
    lens = [len(x) for x in r.reads]
    assert min(lens) >= 66 and sum(ln == 250 for ln in lens) >= 3 and max(lens) == 250 and sum(70 <= ln <= 150 for ln in lens) >= n - 12
    for i in range(n):  # one or more lines per read, in read order, with the read's name, bases and qualities
        chunk = r.sam[int(r.sam_off[i]):int(r.sam_off[i + 1])]
        assert chunk.endswith(b"\n")
        for ln in chunk.splitlines():
            f = ln.split(b"\t")
            flag = int(f[1])
            assert f[0] == r.names[i] and bool(flag & 1) == r.pe
            if r.pe:
                assert bool(flag & 0x80) == bool(i & 1) and bool(flag & 0x40) != bool(i & 1) and r.names[i] == r.names[i ^ 1]
            if not flag & 0x800:
                seq = np.frombuffer(f[9], dtype=np.uint8)
                codes = np.array([b"ACGTN".index(bytes([x])) for x in seq], dtype=np.uint8)
                want = r.reads[i] if not flag & 0x10 else mk.rc(r.reads[i])
                assert np.array_equal(codes, want), (name, i)
                q = r.quals[i]
                assert f[10] == (b"*" if q is None else q if not flag & 0x10 else q[::-1]), (name, i)
    m = g[name + "_opt"]
    second = name.endswith("1")
    assert (int(m["a"]), int(m["b"]), int(m["w"]), int(m["T"]), int(m["o_del"]), int(m["pen_unpaired"])) == ((2, 5, 12, 60, 12, 34) if second else (1, 4, 100, 30, 6, 17))
    assert abs(float(m["split_factor"]) - (1.2 if second else 1.5)) < 1e-6 and int(r.chain_opt["split_len"]) == (23 if second else 28)
    assert bool(int(m["flag"]) & pc.MEM_F_PE) == name.startswith("pe") and (r.quals[0] is not None) == r.pe


@pytest.mark.parametrize("name", pc.RUNS)
def test_shape_counts(name):
    """every shape the tool asserted on the reference's output, counted again from the stored SAM text: flags 0x4, 0x100 and 0x800,
    SA:Z, mapQ 0, an S in the CIGAR, more than 24 CIGAR operations, ... and for rescue the properly paired pairs whose mate no seed
    places (the mutation tag in their name).  Neither option set has -a or -M, under which alone this reference prints flag 0x100:
    that count is stored, and is zero."""
    r, g, w = pc.run(name), pc.fixture(), pc.world()
    offs = np.array([o for o, _ in w.contigs] + [w.l_pac], dtype=np.int64)
    counts = mk.count_shapes(r.sam, r.pe, w.l_pac, offs)
    stored = dict(zip([str(k) for k in g[name + "_shape_names"]], [int(v) for v in g[name + "_shape_counts"]]))
    assert counts == stored, {k: (counts.get(k), stored.get(k)) for k in set(counts) | set(stored) if counts.get(k) != stored.get(k)}
    need = {**mk.MINIMUM, **(mk.MINIMUM_PE if r.pe else {})}
    assert set(need) == set(stored) and not {k: (stored[k], v) for k, v in need.items() if stored[k] < v}
    # independently of the tool's counter, from the columns alone
    lines = [ln.split(b"\t") for ln in r.sam.splitlines()]
    flags = np.array([int(f[1]) for f in lines])
    assert int((flags & 0x4 > 0).sum()) == stored["unmapped"] >= 5 and int((flags & 0x800 > 0).sum()) == stored["flag_0x800"] >= 3
    assert int((flags & 0x100 > 0).sum()) == stored["flag_0x100"] == 0
    assert sum(any(t.startswith(b"SA:Z:") for t in f[11:]) for f in lines) == stored["sa_tag"] >= 2 * stored["flag_0x800"] - 2
    assert sum(int(f[4]) == 0 and not int(f[1]) & 4 for f in lines) == stored["mapq0"] >= 8
    assert sum(b"S" in f[5] for f in lines) == stored["soft_clip"] >= 8
    assert sum(sum(ch in b"MIDS" for ch in f[5]) > 24 for f in lines) == stored["long_cigar"] >= 1
    if r.pe:
        rescued = sum(mk.MUT_TAG in f[0] and int(f[1]) & 0x42 == 0x42 and not int(f[1]) & 0x900 for f in lines)
        assert rescued == stored["rescued"] >= 10


@pytest.mark.ref
@pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", pc.RUNS)
def test_the_reference_gives_the_stored_text_today(name, tmp_path):
    """oracle/_ref/bwa index and mem on the fixture's genome and reads, a plain child process with nothing preloaded"""
    r, w = pc.run(name), pc.world()
    tmp = str(tmp_path)
    fa = os.path.join(tmp, "ref.fa")
    mk.write_fasta(fa, w.genome, np.array([o for o, _ in w.contigs] + [w.l_pac]))
    reflib.build_index(fa)
    files = [os.path.join(tmp, "r1"), os.path.join(tmp, "r2")][:2 if r.pe else 1]
    for m, path in enumerate(files):
        with open(path, "w") as f:
            for i in range(m, len(r.reads), len(files)):
                if r.quals[i] is None:
                    f.write(">" + r.names[i].decode() + "\n" + mk.letters(r.reads[i]) + "\n")
                else:
                    f.write("@" + r.names[i].decode() + "\n" + mk.letters(r.reads[i]) + "\n+\n" + r.quals[i].decode() + "\n")
    body = mk.run_mem(fa, mk.OPTION_ARGS[int(name[2])], files)
    assert body == r.sam
    assert mk.mem_options(mk.OPTION_ARGS[int(name[2])], r.pe).tobytes() == pc.fixture()[name + "_opt"].tobytes()
