"""Whole-pipeline DUT/REF parity on single-end reads past 10 kb under the preload shim with BMH_WIDE_EXT=1: phase 1's long flanks
go to the int32 extension kernel, phase 2's ksw_global2 regions past 10 176 query columns to the band-ring kernel.  SAM must be
byte-identical to the compiled reference's except @PG, and the shim's log must show tasks on both kernels."""
import os
import re

import numpy as np
import pytest

import reflib
import widegen as wg
from test_00_sam_parity import _run, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

CASES = {"20kb": ([], 12, (18000, 22000)), "50kb": ([], 6, (40000, 60000)), "15kb-A4": (["-A", "4"], 10, (14500, 15500))}


@pytest.mark.parametrize("case", list(CASES))
def test_long_read_se_sam_identical_through_phase_2(genome, case):  # noqa: F811
    _, tmp, fa, ref = genome
    scoring, n, lens = CASES[case]
    rng = np.random.default_rng(4400 + len(case))
    reads = wg.long_reads(rng, ref, n, lens)
    fq = os.path.join(tmp, f"long2_{case}.fq")
    reflib.write_fastq(fq, reads, "m")
    extra = ["-t", "4"] + scoring
    ref_sam = _run(fa, [fq], os.path.join(tmp, f"long2_{case}_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, f"long2_{case}_dut.sam"), extra, True, {"BMH_WIDE_EXT": "1", "BMH_VERBOSE": "1"})
    assert len(ref_sam) > n
    assert ref_sam == dut_sam
    err = _run.last_stderr
    m = re.findall(r"wide extension so far: (\d+) extension tasks on the int32 kernel", err)
    assert m and int(m[-1]) > 0, err[-2000:]
    m = re.findall(r"long global alignments so far: (\d+) ksw_global2 tasks on the band-ring kernel", err)
    assert m and int(m[-1]) > 0, err[-2000:]
