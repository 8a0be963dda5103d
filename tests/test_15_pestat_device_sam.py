"""Whole-pipeline DUT/REF parity with mem_pestat's pair walk on the device (BMH_REGS_DEVICE=1 BMH_DEDUP_DEVICE=1 BMH_PESTAT_DEVICE=1:
bmh_seed_chain_regs_batch brings one word per pair down with the regions, under -e it also applies mem_test_and_remove_exact, and the
chunk's serial section is bmh_pestat_from_candidates): SAM byte-identical to the compiled reference's except @PG, PE with mate rescue
at an even batch size, at an odd one the shim rounds up, and with -e; SE keeps the host path.  Runs early (file name) so that the parent
process is GPU-clean."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import kswgen
import reflib
from __graft_entry__ import load_package
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_06_regs_device_sam import _from_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

DEVICE = {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1", "BMH_PESTAT_DEVICE": "1"}
LINE = r"insert-size candidates from the device: (\d+) pairs, (\d+) candidates, (\d+) exact matches removed on the device, (\d+) host bmh_pestat calls"


def _pestat_lines(stderr):
    m = re.findall(LINE, stderr)
    assert m, "the shim did not report the device's insert-size candidates"
    return [tuple(int(x) for x in row) for row in m]


def _exact_pairs(rng, ref, n, L):  # noqa: N803
    """error-free FR pairs: full-length exact matches, which -e discards"""
    r1, r2 = [], []
    for _ in range(n):
        ins = int(rng.integers(250, 450))
        pos = int(rng.integers(0, len(ref) - ins - 60))
        r1.append(ref[pos:pos + L].copy())
        r2.append((3 - ref[pos + ins - L:pos + ins][::-1]).astype(np.uint8))
    return r1, r2


@pytest.fixture(scope="module")
def pe_reads(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 700, 150, False, pair=True, rescue=0.5)
    h1, h2 = _sim_reads(rng, ref, 200, 125, True, pair=True, rescue=0.5)
    e1, e2 = _exact_pairs(rng, ref, 150, 150)
    f1, f2 = os.path.join(tmp, "ps_1.fq"), os.path.join(tmp, "ps_2.fq")
    reflib.write_fastq(f1, r1 + e1 + h1, "c")
    reflib.write_fastq(f2, r2 + e2 + h2, "c")
    return f1, f2, 2 * (len(r1) + len(e1) + len(h1))


@pytest.fixture(scope="module")
def genome_e():
    """A genome for -e.  With MEM_F_NO_EXACT seeding starts at two occurrences (bwamem.c:212), so a read of unique sequence has no
    seed at all; here every 100 bases carry an exact copy of 30 bases from elsewhere: every read has seeds, its own locus wins by far
    (a candidate for mem_pestat), and an error-free read's head region is the full-length exact match that -e discards."""
    rng = np.random.default_rng(151515)
    tmp = tempfile.mkdtemp(prefix="bmh_sam_e_")
    ref = kswgen.rand_seq(rng, 300000)
    for at in range(200, len(ref) - 200, 100):
        src = int(rng.integers(0, len(ref) - 30))
        ref[at:at + 30] = ref[src:src + 30].copy()
    fa = os.path.join(tmp, "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    r1, r2 = _sim_reads(rng, ref, 500, 150, False, pair=True, rescue=0.3)
    e1, e2 = _exact_pairs(rng, ref, 200, 150)
    f1, f2 = os.path.join(tmp, "pe_1.fq"), os.path.join(tmp, "pe_2.fq")
    reflib.write_fastq(f1, r1 + e1, "c")
    reflib.write_fastq(f2, r2 + e2, "c")
    return tmp, fa, f1, f2, 2 * (len(r1) + len(e1))


@pytest.mark.parametrize("exact", [False, True])  # (the shim evens small chunks out into one batch; True: -b to the read, five batches)
def test_pe_no_exact_sam_identical_with_device_drop_exact(genome_e, exact):
    tmp, fa, f1, f2, n = genome_e
    extra = ["-t", "4", "-b", "300", "-e"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ref.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "dut.sam"), extra, True, dict(DEVICE, **({"BMH_BATCH_EXACT": "1"} if exact else {})))
    assert len(ref_sam) >= n and ref_sam == dut_sam
    rows = _pestat_lines(_run.last_stderr)
    print(rows)
    assert sum(r[0] for r in rows) == n // 2
    for pairs, cands, removed, host_calls in rows:
        assert pairs > 0 and cands > 0 and removed > 0 and host_calls == 0, rows
    # the same reads without -e: nothing is removed, on the device or anywhere
    assert _run(fa, [f1, f2], os.path.join(tmp, "ref2.sam"), extra[:-1], False) == _run(fa, [f1, f2], os.path.join(tmp, "dut2.sam"), extra[:-1], True, DEVICE)
    assert all(r[2] == 0 and r[1] > 0 for r in _pestat_lines(_run.last_stderr))


BATCHES = r"insert-size candidates from the device: (\d+) phase-1 batches of up to (\d+) reads \(evened out to (\d+)(, rounded up to an even number)?"


def test_odd_evened_batch_is_rounded_up_so_that_no_pair_straddles(genome):  # noqa: F811
    """The shim evens -b out over the chunk with at least 4 096 reads per batch, so the rounding needs 8 192 reads or more: 4 099 pairs
    at -t 2 -b 4099 are two batches of 4 099 reads, an odd number, which the shim must make 4 100 + 4 098.  (Left at 4 099 a batch
    would split a pair, and the device call refuses an odd batch with collect on.)"""
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 4099, 101, False, pair=True, rescue=0.2)
    f1, f2 = os.path.join(tmp, "ps_big_1.fq"), os.path.join(tmp, "ps_big_2.fq")
    reflib.write_fastq(f1, r1, "c")
    reflib.write_fastq(f2, r2, "c")
    extra = ["-t", "2", "-b", "4099"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ps_ref_big.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "ps_dut_big.sam"), extra, True, DEVICE)
    assert len(ref_sam) >= 8198 and ref_sam == dut_sam
    m = re.findall(BATCHES, _run.last_stderr)
    assert m and all((int(x[0]), int(x[1]), int(x[2]), bool(x[3])) == (2, 4100, 4099, True) for x in m), m
    rows = _pestat_lines(_run.last_stderr)
    assert sum(r[0] for r in rows) == 4099 and all(r[1] > 0 and r[3] == 0 for r in rows), rows


@pytest.mark.parametrize("name,extra,exact", [("even", ["-t", "4", "-b", "300"], False), ("odd_b_one_batch", ["-t", "4", "-b", "301"], False),
                                              # (the shim evens small chunks out into one batch; -b to the read: seven batches)
                                              ("even_to_the_read", ["-t", "4", "-b", "300"], True)])
def test_pe_mate_rescue_sam_identical_with_device_pestat(genome, pe_reads, name, extra, exact):  # noqa: F811
    rng, tmp, fa, ref = genome
    f1, f2, n = pe_reads
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, f"ps_ref_{name}.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, f"ps_dut_{name}.sam"), extra, True, dict(DEVICE, **({"BMH_BATCH_EXACT": "1"} if exact else {})))
    assert len(ref_sam) >= n
    assert ref_sam == dut_sam
    assert _from_device(_run.last_stderr)[0] >= n // 2
    assert re.search(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls", _run.last_stderr)
    rows = _pestat_lines(_run.last_stderr)
    assert sum(r[0] for r in rows) == n // 2
    for pairs, cands, removed, host_calls in rows:
        assert pairs > 0 and cands > 0 and host_calls == 0, rows
        assert removed == 0, rows
    m = re.findall(BATCHES, _run.last_stderr)
    assert m and int(m[-1][0]) == (7 if exact else 1) and not m[-1][3], m


def test_se_keeps_the_host_path(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 600, 150, False)[0] + _sim_reads(rng, ref, 200, 101, True)[0]
    fq = os.path.join(tmp, "ps_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "ps_ref_se.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "ps_dut_se.sam"), extra, True, DEVICE)
    assert len(ref_sam) > len(reads) and ref_sam == dut_sam
    assert not re.search(LINE, _run.last_stderr)
    assert re.search(r"insert-size candidates from the device: off for this chunk \(single-end reads\)", _run.last_stderr)


def test_odd_batch_to_the_read_keeps_the_host_path(genome, pe_reads):  # noqa: F811
    rng, tmp, fa, ref = genome
    f1, f2, n = pe_reads
    extra = ["-t", "4", "-b", "301"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ps_ref_odd.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "ps_dut_odd.sam"), extra, True, dict(DEVICE, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert not re.search(LINE, _run.last_stderr)
    assert re.search(r"off for this chunk \(BMH_BATCH_EXACT=1 with an odd batch size\), 1 host bmh_pestat calls", _run.last_stderr)


def test_switch_without_dedup_device_is_refused_at_load(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    env = dict(os.environ, LD_PRELOAD=load_package().DROPIN_PATH, BMH_REGS_DEVICE="1", BMH_PESTAT_DEVICE="1", BMH_VERBOSE="1")
    env.pop("BMH_DEDUP_DEVICE", None)
    r = subprocess.run([reflib.REF_BWA, "mem", fa, os.path.join(tmp, "missing.fq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 1 and "BMH_PESTAT_DEVICE=1" in err and "BMH_DEDUP_DEVICE=1" in err, (r.returncode, err[-500:])
    assert "[bwamem_hip] the first chunk" not in err and "[M::" not in err  # refused before the program's main ran: no GPU work
