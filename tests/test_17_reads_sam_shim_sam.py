"""Whole-pipeline DUT/REF parity with a single-end chunk's batches going from bases to SAM text in one device session each
(BMH_READS_SAM_DEVICE=1: the shim's mem_process_seqs gives every batch of `-b` reads to bmh_reads_sam_device and cuts the text into the
reads' strings; no region vector, no phase 2 slices).  Single-end inputs of the earlier whole-SAM files under the switch -- plain, many
batches with a first read id that is not 0, options that reach phase 2 and the text, the multi-contig input, on top of every other
device switch, long reads --, the paired-end fixture, which must go the way it goes without the switch, and the refusal at load.  SAM
byte-identical to the compiled reference's except @PG.  Runs early (file name) so that the parent process is GPU-clean."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import kswgen
import reflib
import widegen as wg
from __graft_entry__ import load_package
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_08_matesw_device_sam import pe  # noqa: F401  (the module-scoped fixture: fasta, fastq files, the reference's SAM)
from test_12_phase2_device_sam import EVERY_OTHER

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

ON = {"BMH_READS_SAM_DEVICE": "1"}
SO_FAR = "in one session so far"


def _shim_line(err):
    m = re.findall(r"single-end reads to SAM text in one session so far: (\d+) batches, (\d+) reads, (\d+) regions, (\d+) redone on the host, (\d+) lines, "
                   r"(\d+) bytes\n", err)
    assert m, "the shim did not report the session: " + err[-1500:]
    return tuple(int(x) for x in m[-1])  # (the counts run over the chunks so far)


def _check_line(sam, n_reads):
    """reads, lines and bytes as the SAM has them, no more regions than mapped records; the chunk line of the new form and none of the
    two-phase route's.  Returns the batch count."""
    err = _run.last_stderr
    batches, reads, regions, redone, lines, nbytes = _shim_line(err)
    rec = [l for l in sam if not l.startswith("@")]
    assert (reads, lines, nbytes) == (n_reads, len(rec), sum(len(l) for l in rec)), (reads, lines, nbytes, n_reads, len(rec))
    assert batches >= 1 and redone <= regions
    assert re.search(r"chunk of \d+ reads: reads to SAM text in one session \d+\.\d{3} s\n", err)
    assert "phase 2 (marking, pairing" not in err and "phase 1 so far" not in err and "phase 2 thread-seconds" not in err
    return batches


@pytest.fixture(scope="module")
def se(genome):  # noqa: F811
    """(tmp, fasta, fastq, reads): 700 reads of 150 bases and 300 hard reads of 250, made once for the cases that share them"""
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 700, 150, False)[0] + _sim_reads(rng, ref, 300, 250, True)[0]
    fq = os.path.join(tmp, "rs_se.fq")
    reflib.write_fastq(fq, reads)
    return tmp, fa, fq, reads


def test_se_sam_identical_in_one_session_per_batch(se):
    tmp, fa, fq, reads = se
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rs_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rs_dut.sam"), extra, True, ON)
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    _check_line(dut_sam, len(reads))
    # without the switch the line is not printed, and the two-phase route reports as it always did
    assert ref_sam == _run(fa, [fq], os.path.join(tmp, "rs_dut0.sam"), extra, True)
    assert SO_FAR not in _run.last_stderr and "phase 2 (marking, pairing" in _run.last_stderr


def test_se_many_batches_whose_first_read_is_not_read_0(se):
    """BMH_BATCH_EXACT=1: 16 batches of 65 reads, the last one short (25), then 40 batches of one read; the read ids that mark the
    primary among equal scores (id0 + the read's place) differ from batch to batch"""
    tmp, fa, fq, reads = se
    extra = ["-t", "3", "-b", "65"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rs_ref_b65.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rs_dut_b65.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert _check_line(dut_sam, len(reads)) == -(-len(reads) // 65) == 16
    fq40 = os.path.join(tmp, "rs_se40.fq")
    reflib.write_fastq(fq40, reads[:40])
    extra = ["-t", "3", "-b", "1"]
    ref_sam = _run(fa, [fq40], os.path.join(tmp, "rs_ref_b1.sam"), extra, False)
    dut_sam = _run(fa, [fq40], os.path.join(tmp, "rs_dut_b1.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert _check_line(dut_sam, 40) == 40


@pytest.mark.parametrize("opts", [["-a"], ["-M", "-R", "@RG\\tID:grp.1\\tSM:sample"], ["-e"], ["-A", "2", "-B", "5", "-w", "12", "-r", "1.2"]],
                         ids=["all_alignments", "mark_secondary_and_read_group", "no_exact", "scoring_band_reseeding"])
def test_se_options_that_reach_phase_2_and_the_text(se, opts):
    tmp, fa, fq, reads = se
    extra = ["-t", "4", "-b", "300"] + opts
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rs_ref_opt.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rs_dut_opt.sam"), extra, True, ON)
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    _check_line(dut_sam, len(reads))
    if "-R" in opts:
        rec = [l for l in dut_sam if not l.startswith("@")]
        assert all("\tRG:Z:grp.1" in l for l in rec) and any(l.startswith("@RG") for l in dut_sam)


def test_multi_contig_reference_sam_identical_in_one_session_per_batch():
    """test_14's multi-contig input, rebuilt here: three names in RNAME and SA:Z, reads that hang over contig ends, and the five
    deliberate edge reads; evened-out batches and batches of exactly 200"""
    rng = np.random.default_rng(515151)
    tmp = tempfile.mkdtemp(prefix="bmh_rs_mc_")
    contigs = [kswgen.rand_seq(rng, n) for n in (90000, 30011, 6007)]
    fa = os.path.join(tmp, "mc.fa")
    with open(fa, "w") as f:
        for k, c in enumerate(contigs):
            f.write(f">ctg{k} some description\n")
            s = "".join("ACGT"[b] for b in c)
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + "\n")
    reflib.build_index(fa)
    whole = np.concatenate(contigs)
    reads = []
    for _ in range(600):
        L = int(rng.choice([100, 150, 151, 220]))
        pos = int(rng.integers(0, len(whole) - L))  # may straddle a contig boundary
        rd = kswgen.mutate(rng, whole[pos:pos + L + 10], 0.02, 0.003, 0.003, 3)[:L].copy()
        if rng.random() < 0.5:
            rd = np.where(rd[::-1] > 3, 4, 3 - rd[::-1]).astype(np.uint8)
        reads.append(rd)
    for b in (0, 90000 - 70, 90000 - 20, 120011 - 75, len(whole) - 150):  # deliberately across / at the ends
        reads.append(whole[b:b + 150].copy())
    fq = os.path.join(tmp, "mc.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "3", "-b", "200"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "ref.sam"), extra, False)
    assert len(ref_sam) > len(reads) and len({l.split("\t")[2] for l in ref_sam if not l.startswith("@")} - {"*"}) == 3
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dut.sam"), extra, True, ON)
    assert ref_sam == dut_sam
    _check_line(dut_sam, len(reads))
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dut_exact.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert _check_line(dut_sam, len(reads)) == -(-len(reads) // 200)


def test_se_on_top_of_every_other_device_switch(se):
    """the route consults none of them: the new line is there, theirs are not"""
    tmp, fa, fq, reads = se
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rs_ref.sam"), extra, False)
    env = dict(EVERY_OTHER, BMH_PHASE2_DEVICE="1", BMH_SAMTEXT_DEVICE="1", BMH_PHASE2_TEXT_DEVICE="1", **ON)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rs_dut_all.sam"), extra, True, env)
    assert ref_sam == dut_sam
    _check_line(dut_sam, len(reads))
    assert "phase 2 and SAM text on the device in one session:" not in _run.last_stderr


def test_pe_chunks_go_the_way_they_go_without_the_switch(pe):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "rs_dut_pe.sam"), extra, True, ON)
    assert ref_sam == dut_sam
    err = _run.last_stderr
    assert "single-end reads to SAM text in one session: off for this chunk (paired-end reads)\n" in err
    assert SO_FAR not in err
    assert re.search(r"mate rescue: \d+ pairs, \d+ ksw_align2 calls", err) and "phase 2 (marking, pairing" in err


def test_long_reads_se_sam_identical_in_one_session_per_batch(genome):  # noqa: F811
    """test_03's smaller input, the 30 reads of 8.5 to 9.5 kb at -A 4, all of them kept: every alignment outgrows the region record's
    slots and is finished on the device"""
    _, tmp, fa, ref = genome
    case = "9kb-A4"
    reads = wg.long_reads(np.random.default_rng(4300 + len(case)), ref, 30, (8500, 9500))
    fq = os.path.join(tmp, "rs_long.fq")
    reflib.write_fastq(fq, reads, "l")
    extra = ["-t", "4", "-A", "4"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rs_long_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rs_long_dut.sam"), extra, True, dict(ON, BMH_WIDE_EXT="1", BMH_REGION_LONG="1"))
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    _check_line(dut_sam, len(reads))


def test_refused_at_load_without_the_resident_reference(se):
    tmp, fa, fq, _ = se
    out = os.path.join(tmp, "rs_refused.sam")
    env = dict(os.environ, LD_PRELOAD=load_package().DROPIN_PATH, BMH_PAC_RESIDENT="0", **ON)
    with open(out, "w") as f:
        r = subprocess.run([reflib.REF_BWA, "mem", "-v", "1", "-t", "4", "-b", "300", fa, fq], stdout=f, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode != 0 and os.path.getsize(out) == 0
    assert "[bwamem_hip] fatal: BMH_READS_SAM_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0\n" in r.stderr.decode()
