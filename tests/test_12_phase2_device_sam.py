"""Whole-pipeline DUT/REF parity with phase 2's decisions and alignments as one device session (BMH_PHASE2_DEVICE=1: bmh_sam_batch
takes pass A and pass B from bmh_phase2_device): test_11's three inputs -- the paired-end fixture under the switch alone and on top
of every other device switch, the multi-contig input (reads over contig ends: regions get fixed behind the sort), and a single-end
run with -a (several printed regions per read).  SAM byte-identical to the compiled reference's except @PG.  Runs early (file name)
so that the parent process is GPU-clean."""
import os
import re
import tempfile

import numpy as np
import pytest

import kswgen
import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_08_matesw_device_sam import pe  # noqa: F401  (the module-scoped fixture: fasta, fastq files, the reference's SAM)
from test_09_decide_device_sam import ALL_DEVICE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

EVERY_OTHER = dict(ALL_DEVICE, BMH_DECIDE_DEVICE="1", BMH_WANTED_DEVICE="1")


def _shim_line(err):
    m = re.findall(r"phase 2 on the device in one session: (\d+) units, (\d+) regions, (\d+) fixed, (\d+) redone on the host, (\d+) host fall-backs\n", err)
    assert m, "the shim did not report the fused session"
    return tuple(int(x) for x in m[-1])  # (the counts run over the chunks so far)


def _printed_regions(sam):
    """lines with a CIGAR: every printed region got one alignment"""
    return sum(1 for l in sam if not l.startswith("@") and l.split("\t")[5] != "*")


@pytest.mark.parametrize("more", [{}, EVERY_OTHER], ids=["alone", "with_every_device_switch"])
def test_pe_sam_identical_in_one_session(pe, more):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "p2_dut_pe.sam"), extra, True, dict(more, BMH_PHASE2_DEVICE="1"))
    assert ref_sam == dut_sam
    units, regions, fixed, redone, fallbacks = _shim_line(_run.last_stderr)
    assert regions == _printed_regions(dut_sam) and redone == 0 and fallbacks == 0, (regions, _printed_regions(dut_sam), redone, fallbacks)
    with open(fqs[0]) as f:
        assert units == sum(1 for _ in f) // 4  # every pair went through the fused call


def test_multi_contig_reference_sam_identical_in_one_session():
    """test_00's multi-contig input, rebuilt here: reads that hang over contig ends exercise the fix round"""
    rng = np.random.default_rng(515151)
    tmp = tempfile.mkdtemp(prefix="bmh_p2_mc_")
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
    for _ in range(900):
        L = int(rng.choice([100, 150, 151, 220]))
        pos = int(rng.integers(0, len(whole) - L))  # may straddle a contig boundary
        rd = kswgen.mutate(rng, whole[pos:pos + L + 10], 0.02, 0.003, 0.003, 3)[:L].copy()
        if rng.random() < 0.2:
            rd[rng.random(len(rd)) < 0.02] = 4
        if rng.random() < 0.5:
            rd = np.where(rd[::-1] > 3, 4, 3 - rd[::-1]).astype(np.uint8)
        reads.append(rd)
    for b in (0, 90000 - 70, 90000 - 20, 120011 - 75, len(whole) - 150):  # deliberately across / at the ends
        reads.append(whole[b:b + 150].copy())
    fq = os.path.join(tmp, "mc.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "3", "-b", "200"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dut.sam"), extra, True, {"BMH_PHASE2_DEVICE": "1"})
    assert len(ref_sam) > len(reads) and ref_sam == dut_sam
    units, regions, fixed, redone, fallbacks = _shim_line(_run.last_stderr)
    assert units == len(reads) and regions == _printed_regions(dut_sam) and fixed >= 1 and fallbacks == 0, (units, regions, fixed, fallbacks)
    r1, r2 = _sim_reads(rng, whole, 500, 125, False, pair=True, rescue=0.4)
    f1, f2 = os.path.join(tmp, "mc_1.fq"), os.path.join(tmp, "mc_2.fq")
    reflib.write_fastq(f1, r1, "q")
    reflib.write_fastq(f2, r2, "q")
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "dut_pe.sam"), extra, True, {"BMH_PHASE2_DEVICE": "1"})
    assert len(ref_sam) >= 1000 and ref_sam == dut_sam
    units, regions, fixed, redone, fallbacks = _shim_line(_run.last_stderr)
    assert units == 500 and regions == _printed_regions(dut_sam) and fixed >= 1 and fallbacks == 0, (units, regions, fixed, fallbacks)


def test_se_all_alignments_sam_identical_in_one_session(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 700, 150, False)[0] + _sim_reads(rng, ref, 300, 250, True)[0]
    fq = os.path.join(tmp, "p2_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300", "-a"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "p2_ref_se.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "p2_dut_se.sam"), extra, True, {"BMH_PHASE2_DEVICE": "1"})
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    units, regions, _, _, fallbacks = _shim_line(_run.last_stderr)
    assert units == len(reads) and regions == _printed_regions(dut_sam) and fallbacks == 0
    # without the switch the line is not printed
    _run(fa, [fq], os.path.join(tmp, "p2_dut_se0.sam"), extra, True)
    assert "in one session" not in _run.last_stderr
