"""Whole-pipeline DUT/REF parity with the chains-to-regions driver on the device (BMH_REGS_DEVICE=1: ONE bmh_seed_chain_regs_batch
per batch in place of seeding + chaining + bmh_chains2regs_batch in the shim's phase 1): SAM byte-identical to the compiled
reference's except @PG, SE and PE with mate rescue, on test_00_sam_parity's genome with planted repeats, and on reads whose chains
mem_chain2aln_short takes.  Runs early (file name) so that the parent process is GPU-clean."""
import os
import re

import numpy as np
import pytest

import kswgen
import reflib
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

DEVICE = {"BMH_REGS_DEVICE": "1"}


def _from_device(stderr):
    m = re.findall(r"phase 1 so far: (\d+) chains and regions from bmh_seed_chain_regs_batch on the device, (\d+) seeds extended "
                   r"\(\+\d+ speculated in vain\), (\d+) short-chain", stderr)
    assert m, "the shim did not report the device path"
    for other in ("bmh_chains2regs_batch", "chains from bmh_chain_reads", "chains from bmh_seed_chain_batch", "extension batch"):
        assert other not in stderr, other
    return int(m[-1][0]), int(m[-1][1]), int(m[-1][2])


def _short_chain_reads(rng, ref, n):
    """40-90 genome bases between random flanks of 61-80 bases (mem_chain2aln_short's qualifying test accepts such chains); every
    third read continues the genome into the flanks with mismatches, which its Smith-Waterman then refuses to settle."""
    out = []
    for k in range(n):
        m, f5, f3 = int(rng.integers(40, 91)), int(rng.integers(61, 81)), int(rng.integers(61, 81))
        pos = int(rng.integers(200, len(ref) - 400))
        a, b = kswgen.rand_seq(rng, f5).astype(np.uint8), kswgen.rand_seq(rng, f3).astype(np.uint8)
        if k % 3 == 0:
            l5, l3 = np.array(ref[pos - 30:pos], dtype=np.uint8), np.array(ref[pos + m:pos + m + 30], dtype=np.uint8)
            l5[::9] = (l5[::9] + 1) & 3
            l3[4::9] = (l3[4::9] + 1) & 3
            a[-30:], b[:30] = l5, l3
        r = np.concatenate([a, np.asarray(ref[pos:pos + m], dtype=np.uint8), b]).astype(np.uint8)
        out.append((3 - r[::-1]).astype(np.uint8) if k % 2 else r)
    return out


@pytest.mark.parametrize("extra", [["-t", "4", "-b", "512"], ["-t", "3", "-b", "300", "-k", "14", "-r", "1.0", "-c", "20"],
                                   ["-t", "2", "-b", "64", "-w", "10", "-d", "30"]])
def test_se_sam_identical_with_device_regions(genome, extra):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 1200, 150, False)[0] + _sim_reads(rng, ref, 600, 250, True)[0] + _sim_reads(rng, ref, 300, 101, True)[0]
    fq = os.path.join(tmp, "rd_se.fq")
    reflib.write_fastq(fq, reads)
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rd_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rd_dut.sam"), extra, True, dict(DEVICE, BMH_BATCH_EXACT="1"))
    assert len(ref_sam) > len(reads)
    assert ref_sam == dut_sam
    assert _from_device(_run.last_stderr)[0] >= len(reads) // 2


def test_se_sam_identical_with_short_chain_reads(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads = _sim_reads(rng, ref, 500, 150, False)[0] + _short_chain_reads(rng, ref, 300)
    fq = os.path.join(tmp, "rd_short.fq")
    reflib.write_fastq(fq, reads)
    extra = ["-t", "4", "-b", "256"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rd_short_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rd_short_dut.sam"), extra, True, DEVICE)
    assert ref_sam == dut_sam
    chains, extended, short_sw = _from_device(_run.last_stderr)
    assert short_sw >= 100 and extended > 0 and chains >= 500


def test_pe_mate_rescue_sam_identical_with_device_regions(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(rng, ref, 900, 150, False, pair=True, rescue=0.5)
    h1, h2 = _sim_reads(rng, ref, 300, 125, True, pair=True, rescue=0.5)
    f1, f2 = os.path.join(tmp, "rd_1.fq"), os.path.join(tmp, "rd_2.fq")
    reflib.write_fastq(f1, r1 + h1, "c")
    reflib.write_fastq(f2, r2 + h2, "c")
    extra = ["-t", "4", "-b", "300"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "rd_ref_pe.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "rd_dut_pe.sam"), extra, True, DEVICE)
    assert len(ref_sam) >= 2400
    assert ref_sam == dut_sam
    assert _from_device(_run.last_stderr)[0] >= 1200
    assert re.search(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls", _run.last_stderr)
