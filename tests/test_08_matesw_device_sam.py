"""Whole-pipeline DUT/REF parity with mate rescue's driver on the device (BMH_MATESW_DEVICE=1: bmh_matesw_device plans, folds and
de-duplicates in a kernel, and the shim's mate rescue makes no host dedup callback): PE with mate rescue, SAM byte-identical to the
compiled reference's except @PG, under the switch alone and on top of BMH_REGS_DEVICE=1 BMH_DEDUP_DEVICE=1, on test_00_sam_parity's
genome with planted repeats.  Runs early (file name) so that the parent process is GPU-clean."""
import os
import re
import subprocess

import pytest

import reflib
from __graft_entry__ import load_package
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]


@pytest.fixture(scope="module")
def pe(genome):  # noqa: F811
    """(fasta, the two fastq files, the reference's SAM), made once for both settings"""
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 900, 150, False, pair=True, rescue=0.5)
    h1, h2 = _sim_reads(rng, ref, 300, 125, True, pair=True, rescue=0.5)
    f1, f2 = os.path.join(tmp, "md_1.fq"), os.path.join(tmp, "md_2.fq")
    reflib.write_fastq(f1, r1 + h1, "c")
    reflib.write_fastq(f2, r2 + h2, "c")
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "md_ref_pe.sam"), extra, False)
    assert len(ref_sam) >= 2400
    return tmp, fa, [f1, f2], extra, ref_sam


@pytest.mark.parametrize("more", [{}, {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1"}], ids=["alone", "with_regs_and_dedup_device"])
def test_pe_mate_rescue_sam_identical_with_device_rescue(pe, more):
    tmp, fa, fqs, extra, ref_sam = pe
    dut_sam = _run(fa, fqs, os.path.join(tmp, "md_dut_pe.sam"), extra, True, dict(more, BMH_MATESW_DEVICE="1"))
    assert ref_sam == dut_sam
    err = _run.last_stderr
    m = re.findall(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls in (\d+) GPU rounds, (\d+) pool bytes", err)
    assert m and sum(int(x[1]) for x in m) > 100
    d = re.findall(r"mate rescue on the device: (\d+) active pairs, (\d+) host dedup callbacks", err)
    assert d and len(d) == len(m), "the shim did not report the device driver"
    assert sum(int(x[0]) for x in d) >= 100 and all(int(x[1]) == 0 for x in d), d


def test_matesw_device_without_resident_reference_exits_before_the_gpu(pe):
    tmp, fa, fqs, extra, _ = pe
    env = dict(os.environ, LD_PRELOAD=load_package().DROPIN_PATH, BMH_MATESW_DEVICE="1", BMH_PAC_RESIDENT="0")
    r = subprocess.run([reflib.REF_BWA, "mem", "-v", "1"] + extra + [fa] + fqs, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-500:])
    assert b"BMH_MATESW_DEVICE=1 needs the reference resident" in r.stderr
