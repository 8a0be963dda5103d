"""Whole-pipeline DUT/REF parity at high scores: -A up to 120 on 250 bp reads puts extension and mate-rescue scores near 30 000,
the top of the 16-bit range the kernels accept (l_query * a <= 32000).  -B, -O and -E are given explicitly: with -A alone the
reference would scale them past int8 (the matrix) and 255 (the Smith-Waterman gap costs).  SAM must be byte-identical to the
compiled reference's except @PG, SE and PE with mate rescue."""
import os
import re

import pytest

import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

SCALED = [["-A", "40", "-B", "127", "-O", "150", "-E", "40"], ["-A", "120", "-B", "127", "-O", "130", "-E", "120"]]


def _best_scores(sam):
    return [int(m.group(1)) for l in sam if not l.startswith("@") for m in [re.search(r"\tAS:i:(\d+)", l)] if m]


@pytest.mark.parametrize("scoring", SCALED, ids=["A40", "A120"])
def test_se_sam_identical_at_high_scores(genome, scoring):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 500, 250, False)[0] + _sim_reads(rng, ref, 300, 250, True)[0]
    tag = scoring[1]
    fq = os.path.join(tmp, f"sc{tag}_se.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "300"] + scoring
    ref_sam = _run(fa, [fq], os.path.join(tmp, f"sc{tag}_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, f"sc{tag}_dut.sam"), extra, True)
    assert len(ref_sam) > len(reads)
    assert max(_best_scores(ref_sam)) > 200 * int(scoring[1])  # the scores really are scaled
    assert ref_sam == dut_sam


@pytest.mark.parametrize("scoring", SCALED, ids=["A40", "A120"])
def test_pe_mate_rescue_sam_identical_at_high_scores(genome, scoring):  # noqa: F811
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 500, 250, False, pair=True, rescue=0.5)
    tag = scoring[1]
    f1, f2 = os.path.join(tmp, f"sc{tag}_1.fq"), os.path.join(tmp, f"sc{tag}_2.fq")
    reflib.write_fastq(f1, r1, "s")
    reflib.write_fastq(f2, r2, "s")
    extra = ["-t", "4", "-b", "200"] + scoring
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, f"sc{tag}_ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, f"sc{tag}_dut_pe.sam"), extra, True)
    assert len(ref_sam) >= 1000
    assert max(_best_scores(ref_sam)) > 200 * int(scoring[1])
    assert ref_sam == dut_sam
    m = re.findall(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls", _run.last_stderr)
    assert m and sum(int(x[1]) for x in m) > 0  # mate rescue ran, at these scores through word-mode ksw_align2
