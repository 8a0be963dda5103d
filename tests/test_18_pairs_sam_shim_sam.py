"""Whole-pipeline DUT/REF parity with a paired-end chunk's batches going from bases to SAM text in device sessions parked at the
insert-size barrier (BMH_PAIRS_SAM_DEVICE=1: the shim's mem_process_seqs begins every batch with bmh_pairs_sam_begin, makes the chunk's
table from all batches' words, and finishes every batch with bmh_pairs_sam_finish; no region vector, no phase 2 slices).  test_08's
paired-end input under the switch -- one batch, many batches under one table, an odd exact batch size (off), options that reach phase
2 and the text, -I (one pass, nothing parked), -P and -S (off) -- and a single-end input with both one-session switches on, which goes the
sibling's way.  SAM byte-identical to the compiled reference's except @PG.  Runs early (file name) so that the parent process is
GPU-clean."""
import os
import re

import pytest

import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_08_matesw_device_sam import pe  # noqa: F401  (the module-scoped fixture: fasta, fastq files, the reference's SAM)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

ON = {"BMH_PAIRS_SAM_DEVICE": "1"}
SO_FAR = "paired-end reads to SAM text in one session so far"
OFF = "paired-end reads to SAM text in one session: off for this chunk (%s)\n"


def _shim_line(err):
    m = re.findall(r"paired-end reads to SAM text in one session so far: (\d+) batches, (\d+) pairs, (\d+) regions, (\d+) after rescue, (\d+) ksw_align2 calls, "
                   r"(\d+) redone on the host, (\d+) lines, (\d+) bytes, (\d+) bytes parked at the barrier\n", err)
    assert m, "the shim did not report the session: " + err[-1500:]
    return tuple(int(x) for x in m[-1])  # (the counts run over the chunks so far)


def _check_line(sam, parked=True):
    """pairs, lines and bytes as the SAM has them; rescue was live; the chunk line of the new form with its three spans (or the
    one-pass form's) and none of the two-phase route's.  Returns (batches, ksw_align2 calls)."""
    err = _run.last_stderr
    batches, pairs, regions, after, n_sw, redone, lines, nbytes, at_barrier = _shim_line(err)
    rec = [l for l in sam if not l.startswith("@")]
    assert (lines, nbytes) == (len(rec), sum(len(l) for l in rec)), (lines, nbytes, len(rec))
    assert 2 * pairs == len({l.split("\t")[0] for l in rec}) * 2 and batches >= 1 and redone <= after and after >= regions > 0
    if parked:
        assert re.search(r"chunk of \d+ reads: pairs to SAM text in parked sessions, \d+ batches of up to \d+ reads: pass 1 \d+\.\d{3} s, table \d+\.\d{3} s, "
                         r"pass 2 \d+\.\d{3} s\n", err), err[-1500:]
        assert at_barrier > 125 * 2 * pairs  # at least the bases: reads of 125 and 150
    else:
        assert re.search(r"chunk of \d+ reads: pairs to SAM text in one session per batch under the given table, \d+ batches of up to \d+ reads, \d+\.\d{3} s\n", err)
        assert at_barrier == 0
    assert "phase 2 (marking, pairing" not in err and "phase 1 so far" not in err and "phase 2 thread-seconds" not in err and "mate rescue:" not in err
    return batches, n_sw


def test_pe_sam_identical_in_parked_sessions(pe):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut.sam"), extra, True, ON)
    assert ref_sam == dut_sam
    batches, n_sw = _check_line(dut_sam)
    assert n_sw > 100  # test_08's input: half of the pairs need rescue


def test_pe_many_batches_under_the_chunks_table(pe):  # noqa: F811
    """BMH_BATCH_EXACT=1 -b 66: 37 batches of 33 pairs, whose own tables would differ from the chunk's; the read ids that mark the
    primary among equal scores differ from batch to batch"""
    tmp, fa, fqs, _, _ = pe
    extra = ["-t", "4", "-b", "66"]
    ref_sam = _run(fa, fqs, os.path.join(tmp, "ps_ref_b66.sam"), extra, False)
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut_b66.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert _check_line(dut_sam)[0] == -(-2400 // 66) == 37


def test_pe_an_odd_exact_batch_size_is_off(pe):  # noqa: F811
    tmp, fa, fqs, _, _ = pe
    extra = ["-t", "4", "-b", "65"]
    ref_sam = _run(fa, fqs, os.path.join(tmp, "ps_ref_b65.sam"), extra, False)
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut_b65.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    err = _run.last_stderr
    assert OFF % "BMH_BATCH_EXACT=1 with an odd batch size" in err and SO_FAR not in err
    assert re.search(r"mate rescue: \d+ pairs, \d+ ksw_align2 calls", err) and "phase 2 (marking, pairing" in err


@pytest.mark.parametrize("opts", [["-a"], ["-M", "-R", "@RG\\tID:grp.1\\tSM:sample"], ["-e"], ["-A", "2", "-B", "5", "-w", "12", "-r", "1.2"]],
                         ids=["all_alignments", "mark_secondary_and_read_group", "no_exact", "scoring_band_reseeding"])
def test_pe_options_that_reach_phase_2_and_the_text(pe, opts):  # noqa: F811
    tmp, fa, fqs, extra, _ = pe
    extra = extra + opts
    ref_sam = _run(fa, fqs, os.path.join(tmp, "ps_ref_opt.sam"), extra, False)
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut_opt.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert len(ref_sam) >= 2400
    assert ref_sam == dut_sam
    assert _check_line(dut_sam)[0] == 8
    if "-R" in opts:
        rec = [l for l in dut_sam if not l.startswith("@")]
        assert all("\tRG:Z:grp.1" in l for l in rec) and any(l.startswith("@RG") for l in dut_sam)


def test_pe_given_table_is_one_pass(pe):  # noqa: F811
    """-I 300,50: the table is the caller's, so there is no barrier: one bmh_pairs_sam_device per batch, nothing parked"""
    tmp, fa, fqs, extra, _ = pe
    extra = extra + ["-I", "300,50"]
    ref_sam = _run(fa, fqs, os.path.join(tmp, "ps_ref_I.sam"), extra, False)
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut_I.sam"), extra, True, dict(ON, BMH_BATCH_EXACT="1"))
    assert ref_sam == dut_sam
    assert _check_line(dut_sam, parked=False)[0] == 8
    assert "in parked sessions" not in _run.last_stderr


@pytest.mark.parametrize("flag,why", [("-P", "-P: no pairing"), ("-S", "-S: the session always runs mate rescue")])
def test_pe_without_pairing_or_rescue_is_off(pe, flag, why):  # noqa: F811
    tmp, fa, fqs, extra, _ = pe
    extra = extra + [flag]
    ref_sam = _run(fa, fqs, os.path.join(tmp, "ps_ref_P.sam"), extra, False)
    dut_sam = _run(fa, fqs, os.path.join(tmp, "ps_dut_P.sam"), extra, True, ON)
    assert ref_sam == dut_sam
    err = _run.last_stderr
    assert OFF % why in err and SO_FAR not in err and "phase 2 (marking, pairing" in err


def test_se_with_both_switches_goes_the_siblings_way(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 400, 150, False)[0]
    fq = os.path.join(tmp, "ps_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "ps_se_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "ps_se_dut.sam"), extra, True, dict(ON, BMH_READS_SAM_DEVICE="1"))
    assert ref_sam == dut_sam
    err = _run.last_stderr
    assert re.search(r"single-end reads to SAM text in one session so far: \d+ batches, 400 reads, ", err)
    assert re.search(r"chunk of 400 reads: reads to SAM text in one session \d+\.\d{3} s\n", err)
    assert "paired-end reads to SAM text" not in err and "phase 2 (marking, pairing" not in err
