"""Whole-pipeline DUT/REF parity with phase 2's decisions on the device (BMH_DECIDE_DEVICE=1: bmh_sam_batch takes primary marking,
pairing, mapQ and the list of regions that get printed from bmh_decide_device): test_08's paired-end input with mate rescue plus
one single-end run, SAM byte-identical to the compiled reference's except @PG, under the switch alone and on top of
BMH_REGS_DEVICE=1 BMH_DEDUP_DEVICE=1 BMH_MATESW_DEVICE=1.  Runs early (file name) so that the parent process is GPU-clean."""
import os
import re

import pytest

import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_08_matesw_device_sam import pe  # noqa: F401  (the module-scoped fixture: fasta, fastq files, the reference's SAM)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

ALL_DEVICE = {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1", "BMH_MATESW_DEVICE": "1"}


def _shim_line(err):
    m = re.findall(r"phase 2 decisions on the device: (\d+) units, (\d+) host fall-backs", err)
    assert m, "the shim did not report the device decisions"
    return int(m[-1][0]), int(m[-1][1])  # (the counts run over the chunks so far)


@pytest.mark.parametrize("more", [{}, ALL_DEVICE], ids=["alone", "with_every_device_switch"])
def test_pe_sam_identical_with_device_decisions(pe, more):  # noqa: F811
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "dd_dut_pe.sam"), extra, True, dict(more, BMH_DECIDE_DEVICE="1"))
    assert ref_sam == dut_sam
    units, fallbacks = _shim_line(_run.last_stderr)
    assert units == 1200 and fallbacks == 0, (units, fallbacks)  # every pair


@pytest.mark.parametrize("more", [{}, {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1"}], ids=["alone", "with_regs_and_dedup_device"])
def test_se_sam_identical_with_device_decisions(genome, more):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 900, 150, False)[0] + _sim_reads(rng, ref, 400, 250, True)[0]
    fq = os.path.join(tmp, "dd_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "dd_ref_se.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dd_dut_se.sam"), extra, True, dict(more, BMH_DECIDE_DEVICE="1"))
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    units, fallbacks = _shim_line(_run.last_stderr)
    assert units == len(reads) and fallbacks == 0, (units, fallbacks)
    # without the switch the line is not printed
    _run(fa, [fq], os.path.join(tmp, "dd_dut_se0.sam"), extra, True)
    assert "decisions on the device" not in _run.last_stderr
