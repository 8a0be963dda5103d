"""Whole-pipeline DUT/REF parity with the regions sorted and de-duplicated on the device (BMH_REGS_DEVICE=1 BMH_DEDUP_DEVICE=1:
bmh_seed_chain_regs_batch returns what mem_sort_and_dedup leaves, and the shim's phase 1 makes no host bmh_sort_and_dedup call): SAM
byte-identical to the compiled reference's except @PG, SE and PE with mate rescue, on test_00_sam_parity's genome with planted
repeats.  Runs early (file name) so that the parent process is GPU-clean."""
import os
import re

import pytest

import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_06_regs_device_sam import _from_device

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

DEVICE = {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1"}


def _dedup_line(stderr):
    m = re.findall(r"region de-duplication so far: (\d+) regions de-duplicated on the device, (\d+) kept, (\d+) host bmh_sort_and_dedup calls in phase 1",
                   stderr)
    assert m, "the shim did not report the device de-duplication"
    return int(m[-1][0]), int(m[-1][1]), int(m[-1][2])


@pytest.mark.parametrize("extra", [["-t", "4", "-b", "512"], ["-t", "3", "-b", "300", "-k", "14", "-r", "1.0", "-c", "20"]])
def test_se_sam_identical_with_device_dedup(genome, extra):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 1200, 150, False)[0] + _sim_reads(rng, ref, 600, 250, True)[0] + _sim_reads(rng, ref, 300, 101, True)[0]
    fq = os.path.join(tmp, "dd_se.fq")
    reflib.write_fastq(fq, reads)
    ref_sam = _run(fa, [fq], os.path.join(tmp, "dd_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "dd_dut.sam"), extra, True, dict(DEVICE, BMH_BATCH_EXACT="1"))
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    assert _from_device(_run.last_stderr)[0] >= len(reads) // 2
    n_in, n_kept, host_calls = _dedup_line(_run.last_stderr)
    assert n_in > n_kept > 0 and host_calls == 0, (n_in, n_kept, host_calls)


def test_pe_mate_rescue_sam_identical_with_device_dedup(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 900, 150, False, pair=True, rescue=0.5)
    h1, h2 = _sim_reads(rng, ref, 300, 125, True, pair=True, rescue=0.5)
    f1, f2 = os.path.join(tmp, "dd_1.fq"), os.path.join(tmp, "dd_2.fq")
    reflib.write_fastq(f1, r1 + h1, "c")
    reflib.write_fastq(f2, r2 + h2, "c")
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "dd_ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "dd_dut_pe.sam"), extra, True, DEVICE)
    assert len(ref_sam) >= 2400
    assert ref_sam == dut_sam
    assert _from_device(_run.last_stderr)[0] >= 1200
    assert re.search(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls", _run.last_stderr)
    n_in, n_kept, host_calls = _dedup_line(_run.last_stderr)
    assert n_in > n_kept > 0 and host_calls == 0, (n_in, n_kept, host_calls)
