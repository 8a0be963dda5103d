"""Whole-pipeline DUT/REF parity with all of phase 2 as one device session (BMH_PHASE2_TEXT_DEVICE=1: bmh_sam_batch takes its three passes
from bmh_phase2_text_device, the regions and reads go up once and only SAM text comes down): test_13's inputs -- the paired-end fixture
under the switch alone and on top of every other device switch, the multi-contig input (several sequence names, reads over contig ends:
the fix round), a single-end run with -a (several printed regions per read) -- and one run with -M and a read group.  SAM
byte-identical to the compiled reference's except @PG.  Runs early (file name) so that the parent process is GPU-clean."""
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
from test_08_matesw_device_sam import pe  # noqa: F401  (the module-scoped fixture: fasta, fastq files, the reference's SAM)
from test_12_phase2_device_sam import EVERY_OTHER

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

ON = {"BMH_PHASE2_TEXT_DEVICE": "1"}


def _shim_line(err):
    m = re.findall(r"phase 2 and SAM text on the device in one session: (\d+) units, (\d+) regions, (\d+) redone on the host, (\d+) lines, (\d+) bytes, "
                   r"(\d+) host fall-backs\n", err)
    assert m, "the shim did not report the fused session"
    return tuple(int(x) for x in m[-1])  # (the counts run over the chunks so far)


def _check_line(sam, fqs):
    """units x reads per unit, lines and bytes as the SAM has them; no more regions than mapped records; nothing fell back"""
    units, regions, redone, lines, nbytes, fallbacks = _shim_line(_run.last_stderr)
    rec = [l for l in sam if not l.startswith("@")]
    n_reads = 0
    for fq in fqs:
        with open(fq) as f:
            n_reads += sum(1 for _ in f) // 4
    assert (units * len(fqs), lines, nbytes, fallbacks) == (n_reads, len(rec), sum(len(l) for l in rec), 0), (units, lines, nbytes, fallbacks, n_reads, len(rec))
    assert redone <= regions <= sum(1 for l in rec if not int(l.split("\t")[1]) & 4)


@pytest.mark.parametrize("more", [{}, dict(EVERY_OTHER, BMH_PHASE2_DEVICE="1", BMH_SAMTEXT_DEVICE="1")], ids=["alone", "with_every_device_switch"])
def test_pe_sam_identical_in_one_session_through_to_the_text(pe, more):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "pt_dut_pe.sam"), extra, True, dict(more, **ON))
    assert ref_sam == dut_sam
    _check_line(dut_sam, fqs)


def test_multi_contig_reference_sam_identical_in_one_session_through_to_the_text():
    """test_00's multi-contig input, rebuilt here: three names in RNAME, RNEXT and SA:Z, reads that hang over contig ends"""
    rng = np.random.default_rng(515151)
    tmp = tempfile.mkdtemp(prefix="bmh_pt_mc_")
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
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dut.sam"), extra, True, ON)
    assert len(ref_sam) > len(reads) and ref_sam == dut_sam
    _check_line(dut_sam, [fq])
    r1, r2 = _sim_reads(rng, whole, 400, 125, False, pair=True, rescue=0.4)
    f1, f2 = os.path.join(tmp, "mc_1.fq"), os.path.join(tmp, "mc_2.fq")
    reflib.write_fastq(f1, r1, "q")
    reflib.write_fastq(f2, r2, "q")
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "dut_pe.sam"), extra, True, ON)
    assert len(ref_sam) >= 800 and ref_sam == dut_sam
    _check_line(dut_sam, [f1, f2])
    # the switch needs the resident reference: refused when the library is loaded, with the message and no SAM
    out = os.path.join(tmp, "refused.sam")
    env = dict(os.environ, LD_PRELOAD=load_package().DROPIN_PATH, BMH_PAC_RESIDENT="0", **ON)
    with open(out, "w") as f:
        r = subprocess.run([reflib.REF_BWA, "mem", "-v", "1"] + extra + [fa, fq], stdout=f, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode != 0 and os.path.getsize(out) == 0
    assert "BMH_PHASE2_TEXT_DEVICE=1 needs the reference resident on the device: BMH_PAC_RESIDENT must not be 0" in r.stderr.decode()


def test_se_all_alignments_and_read_group_sam_identical_in_one_session_through_to_the_text(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 700, 150, False)[0] + _sim_reads(rng, ref, 300, 250, True)[0]
    fq = os.path.join(tmp, "pt_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300", "-a"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "pt_ref_se.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "pt_dut_se.sam"), extra, True, ON)
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    _check_line(dut_sam, [fq])
    # without the switch the line is not printed
    _run(fa, [fq], os.path.join(tmp, "pt_dut_se0.sam"), extra, True)
    assert "in one session:" not in _run.last_stderr
    # -M (a supplementary hit is shown as secondary) and a read group
    extra = ["-t", "4", "-b", "300", "-M", "-R", "@RG\\tID:grp.1\\tSM:sample"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "pt_ref_rg.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "pt_dut_rg.sam"), extra, True, ON)
    assert ref_sam == dut_sam
    assert sum("\tRG:Z:grp.1" in l for l in dut_sam) >= len(reads) and any(l.startswith("@RG") for l in dut_sam)
    _check_line(dut_sam, [fq])
