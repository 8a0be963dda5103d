"""Whole-pipeline DUT/REF parity with BMH_REGION_LONG=1: on single-end reads of 5-20 kb every printed alignment outgrows the region
record's 24 CIGAR words, and the shim finishes them on the device instead of redoing them with host copies.  SAM must be
byte-identical to the compiled reference's except @PG; REF's SAM alone says how many such records there are, and the shim's log
must report at least that many finished on the device and none with host copies.  On 150 bp pairs the switch changes nothing and
no region is long."""
import os
import re

import numpy as np
import pytest

import reflib
import widegen as wg
from test_00_sam_parity import _run, _sim_reads, genome  # noqa: F401  (genome: the module-scoped fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

LINE = re.compile(r"long region records so far: (\d+) regions finished on the device, (\d+) redone with host copies")


def _long_records(sam):
    """per read name, the records of REF's SAM with more than 24 M/I/D operations"""
    by = {}
    for l in sam:
        if l.startswith("@"):
            continue
        f = l.split("\t")
        by.setdefault(f[0], 0)
        if f[5] != "*" and len(re.findall(r"\d+[MID]", f[5])) > 24:
            by[f[0]] += 1
    return by


def test_long_read_se_sam_identical_with_regions_finished_on_the_device(genome):  # noqa: F811
    _, tmp, fa, ref = genome
    rng = np.random.default_rng(1616)
    n = 8
    reads = wg.long_reads(rng, ref, n, (5000, 20000))
    fq = os.path.join(tmp, "rlong.fq")
    reflib.write_fastq(fq, reads, "m")
    extra = ["-t", "4"]
    ref_sam = _run(fa, [fq], os.path.join(tmp, "rlong_ref.sam"), extra, False)
    dut_sam = _run(fa, [fq], os.path.join(tmp, "rlong_dut.sam"), extra, True, {"BMH_WIDE_EXT": "1", "BMH_REGION_LONG": "1", "BMH_VERBOSE": "1"})
    assert len(ref_sam) > n
    assert ref_sam == dut_sam
    by = _long_records(ref_sam)
    assert len(by) == n and min(by.values()) >= 1, by  # from REF alone: every read has a record past the slots
    m = LINE.findall(_run.last_stderr)
    assert m and int(m[-1][0]) >= sum(by.values()) and int(m[-1][1]) == 0, (m[-1:], by, _run.last_stderr[-2000:])


def test_short_pairs_unchanged_and_nothing_long(genome):  # noqa: F811
    rng, tmp, fa, ref = genome
    r1, r2 = _sim_reads(np.random.default_rng(1617), ref, 400, 150, False, pair=True)
    f1, f2 = os.path.join(tmp, "rlong_pe_1.fq"), os.path.join(tmp, "rlong_pe_2.fq")
    reflib.write_fastq(f1, r1, "p")
    reflib.write_fastq(f2, r2, "p")
    extra = ["-t", "4", "-b", "400"]
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, "rlong_pe_ref.sam"), extra, False)
    dut_sam = _run(fa, [f1, f2], os.path.join(tmp, "rlong_pe_dut.sam"), extra, True, {"BMH_REGION_LONG": "1", "BMH_VERBOSE": "1"})
    assert len(ref_sam) >= 800
    assert ref_sam == dut_sam
    assert max(_long_records(ref_sam).values()) == 0
    m = LINE.findall(_run.last_stderr)
    assert m and (int(m[-1][0]), int(m[-1][1])) == (0, 0), m[-1:]
