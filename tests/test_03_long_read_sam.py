"""Whole-pipeline DUT/REF parity on long single-end reads under the preload shim with BMH_WIDE_EXT=1: flanks past the 16-bit
extension kernels' range (9 kb reads at -A 4, 4 kb reads at -A 10) go to the int32 extension kernel.  (Reads past ~10 kb stop in
phase 2 whatever the switch: ksw_global2's wave kernel holds 16 bytes per query column in LDS, 10 176 columns.)  SAM must be
byte-identical to the compiled reference's except @PG, and the shim's log must show extension tasks on the int32 kernel.
Without the switch the shim stops on these reads (BMH_E_RANGE)."""
import os
import re

import numpy as np
import pytest

import reflib
import widegen as wg
from test_00_sam_parity import _run, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

CASES = {"9kb-A4": (["-A", "4"], 30, (8500, 9500)), "4kb-A10": (["-A", "10", "-B", "40", "-O", "60", "-E", "10"], 40, (4000, 4200))}


@pytest.mark.parametrize("case", list(CASES))
def test_long_read_se_sam_identical_with_wide_extension(genome, case):  # noqa: F811
    _, tmp, fa, ref = genome
    scoring, n, lens = CASES[case]
    rng = np.random.default_rng(4300 + len(case))
    reads = wg.long_reads(rng, ref, n, lens)
    fq = os.path.join(tmp, f"long_{case}.fq")
    reflib.write_fastq(fq, reads, "l")
    extra = ["-t", "4"] + scoring
    ref_sam = _run(fa, [fq], os.path.join(tmp, f"long_{case}_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, f"long_{case}_dut.sam"), extra, True, {"BMH_WIDE_EXT": "1"})
    assert len(ref_sam) > n
    assert ref_sam == dut_sam
    m = re.findall(r"wide extension so far: (\d+) extension tasks on the int32 kernel", _run.last_stderr)
    assert m and int(m[-1]) > 0, _run.last_stderr[-2000:]
