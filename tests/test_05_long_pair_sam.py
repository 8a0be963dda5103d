"""Whole-pipeline DUT/REF parity on paired-end long reads under the preload shim with BMH_WIDE_EXT=1: one mate of many pairs is
unseedable (a substitution every 18 bases), so mate rescue has to place it with ksw_align2 on a window of the reference.  Under
-A 4 those calls have qlen*max(mat) past 32000 and run on the long-query Smith-Waterman kernel (the shim turns
bmh_ctx_set_wide_sw on); under the default scoring they are in range and change kernel only.  SAM must be byte-identical to the
compiled reference's except @PG, and the shim's log must show tasks on the new kernel.  Inserts stay below max_ins = 10 000
(bwamem.c:62)."""
import os
import re

import numpy as np
import pytest

import reflib
import widesw as ws
from test_00_sam_parity import _run, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

# scoring, pairs, of which rescued, mate lengths, fragment lengths
CASES = {"8kb-A4": (["-A", "4"], 30, 12, (8000, 8800), (9000, 9900)),
         "4kb": ([], 36, 14, (3000, 5000), (5500, 9000))}


@pytest.mark.parametrize("case", list(CASES))
def test_long_pair_sam_identical_through_mate_rescue(genome, case):  # noqa: F811
    _, tmp, fa, ref = genome
    scoring, n, n_resc, mates, frags = CASES[case]
    rng = np.random.default_rng(4500 + len(case))
    r1, r2 = ws.long_pairs(rng, ref, n, mates, frags, n_resc)
    f1, f2 = os.path.join(tmp, f"lp_{case}_1.fq"), os.path.join(tmp, f"lp_{case}_2.fq")
    reflib.write_fastq(f1, r1, "p")
    reflib.write_fastq(f2, r2, "p")
    extra = ["-t", "4"] + scoring
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, f"lp_{case}_ref.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, f"lp_{case}_dut.sam"), extra, True, {"BMH_WIDE_EXT": "1", "BMH_VERBOSE": "1"})
    recs = [l.split("\t") for l in ref_sam if not l.startswith("@")]
    assert len(recs) >= 2 * n
    # rescue really placed the unseedable mates: mapped second mates of the last n_resc pairs
    placed = sum(1 for x in recs if int(x[1]) & 0x80 and not int(x[1]) & 0x4 and int(x[0][1:]) >= n - n_resc)
    assert placed >= n_resc // 2, placed
    assert ref_sam == dut_sam
    m = re.findall(r"wide Smith-Waterman so far: (\d+) ksw_align2 tasks on the long-query kernel", _run.last_stderr)
    assert m and int(m[-1]) > 0, _run.last_stderr[-2000:]
