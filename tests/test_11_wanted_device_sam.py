"""Whole-pipeline DUT/REF parity with phase 2's alignments planned on the device (BMH_WANTED_DEVICE=1: bmh_sam_batch takes pass B --
the bwa_fix_xref2 test and cut, bands, region records and tasks -- from bmh_wanted_cigar_device): test_09's paired-end input under the
switch alone and on top of every other device switch, the multi-contig input of test_00 (reads over contig ends: regions get fixed),
and a single-end run with -a (several printed regions per read).  SAM byte-identical to the compiled reference's except @PG.  Runs
early (file name) so that the parent process is GPU-clean.  The paired-end input holds a mate that only rescue could place whose MD
is 105 bytes long, the longest of its 2 459 printed regions: no region may be redone on the host for it."""
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

EVERY_OTHER = dict(ALL_DEVICE, BMH_DECIDE_DEVICE="1")


def _shim_line(err):
    m = re.findall(r"phase 2 alignments planned on the device: (\d+) regions, (\d+) fixed, (\d+) redone on the host\n", err)
    assert m, "the shim did not report the device planning"
    return tuple(int(x) for x in m[-1])  # (the counts run over the chunks so far)


def _long_lines(sam):
    """printed regions whose MD is longer than 96 bytes or whose alignment has more than 24 M/I/D operations"""
    n = 0
    for l in sam:
        f = l.split("\t")
        if l.startswith("@") or f[5] == "*":
            continue
        md = [x[5:] for x in f[11:] if x.startswith("MD:Z:")]
        n += (md and len(md[0].strip()) > 96) or len(re.findall(r"\d+[MID]", f[5])) > 24
    return n


def _printed_regions(sam):
    """lines with a CIGAR: every printed region got one alignment"""
    return sum(1 for l in sam if not l.startswith("@") and l.split("\t")[5] != "*")


@pytest.mark.parametrize("more", [{}, EVERY_OTHER], ids=["alone", "with_every_device_switch"])
def test_pe_sam_identical_with_device_planning(pe, more):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "wd_dut_pe.sam"), extra, True, dict(more, BMH_WANTED_DEVICE="1"))
    assert ref_sam == dut_sam
    regions, fixed, redone = _shim_line(_run.last_stderr)
    print(f"regions {regions}, fixed {fixed}, redone {redone}; printed {_printed_regions(dut_sam)}, long MD or CIGAR {_long_lines(dut_sam)}")
    assert regions == _printed_regions(dut_sam) and redone == 0, (regions, _printed_regions(dut_sam), redone, _long_lines(dut_sam))


def test_multi_contig_reference_sam_identical_with_device_planning():
    """test_00's multi-contig input, rebuilt here: reads that hang over contig ends exercise the fix round"""
    rng = np.random.default_rng(515151)
    tmp = tempfile.mkdtemp(prefix="bmh_wd_mc_")
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
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dut.sam"), extra, True, {"BMH_WANTED_DEVICE": "1"})
    assert len(ref_sam) > len(reads) and ref_sam == dut_sam
    regions, fixed, redone = _shim_line(_run.last_stderr)
    assert regions == _printed_regions(dut_sam) and fixed >= 1, (regions, fixed)
    r1, r2 = _sim_reads(rng, whole, 500, 125, False, pair=True, rescue=0.4)
    f1, f2 = os.path.join(tmp, "mc_1.fq"), os.path.join(tmp, "mc_2.fq")
    reflib.write_fastq(f1, r1, "q")
    reflib.write_fastq(f2, r2, "q")
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "dut_pe.sam"), extra, True, {"BMH_WANTED_DEVICE": "1"})
    assert len(ref_sam) >= 1000 and ref_sam == dut_sam
    regions, fixed, redone = _shim_line(_run.last_stderr)
    assert regions == _printed_regions(dut_sam) and fixed >= 1, (regions, fixed)


def test_se_all_alignments_sam_identical_with_device_planning(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 700, 150, False)[0] + _sim_reads(rng, ref, 300, 250, True)[0]
    fq = os.path.join(tmp, "wd_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300", "-a"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "wd_ref_se.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "wd_dut_se.sam"), extra, True, {"BMH_WANTED_DEVICE": "1"})
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    assert _shim_line(_run.last_stderr)[0] == _printed_regions(dut_sam)
    # without the switch the line is not printed
    _run(fa, [fq], os.path.join(tmp, "wd_dut_se0.sam"), extra, True)
    assert "planned on the device" not in _run.last_stderr
