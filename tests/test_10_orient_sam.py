"""Whole-pipeline DUT/REF parity on libraries that are not FR: 1 200 pairs of 150 bp with the mate in each of the four orientations of
mem_infer_dir (tests/orientgen.read_pairs4; half of the mates too noisy to seed, so mate rescue places them), and a pure RF
(mate-pair) library with an insert of 2 000-3 000.  The shim's bmh_pestat then opens three or four orientations, mate rescue finds
mates that are not reverse-complemented or lie upstream, and the proper-pair decisions of bmh_sam_batch run over several windows:
SAM byte-identical to the compiled reference's except @PG, on the host paths and with every device switch on
(BMH_REGS_DEVICE, BMH_DEDUP_DEVICE, BMH_MATESW_DEVICE, BMH_DECIDE_DEVICE).  Runs early (file name) so that the parent process is
GPU-clean."""
import os
import re

import pytest

import orientgen as og
import reflib
from test_00_sam_parity import _run, genome  # noqa: F401  (genome: the module-scoped fixture)
from test_06_regs_device_sam import _from_device
from test_07_dedup_device_sam import _dedup_line
from test_09_decide_device_sam import _shim_line

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")]

EVERY_DEVICE = {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1", "BMH_MATESW_DEVICE": "1", "BMH_DECIDE_DEVICE": "1"}
EXTRA = ["-t", "4", "-b", "300"]
N_PAIRS = 1200


def proper_pairs_by_orientation(sam):
    """Properly paired primary records of read 1 per orientation, from the strands (0x10, 0x20) and the two leftmost positions.  On
    read 1's strand (mem_infer_dir): one strand and the mate ahead is FF, behind RR; opposite strands and the mate ahead is FR,
    behind RF -- where `ahead` means a larger leftmost position for a forward read 1 and a smaller one for a reverse read 1."""
    n = [0] * 4
    for line in sam:
        if line.startswith("@"):
            continue
        f = line.split("\t")
        flag = int(f[1])
        if not flag & 0x2 or not flag & 0x40 or flag & 0x900:
            continue
        rev1, rev2 = bool(flag & 0x10), bool(flag & 0x20)
        ahead = int(f[7]) > int(f[3]) if not rev1 else int(f[7]) < int(f[3])
        n[(0 if rev1 == rev2 else 1) ^ (0 if ahead else 3)] += 1
    return n


def _library(genome, name, mix, dists):  # noqa: F811
    rng, tmp, fa, ref = genome
    reads, _ = og.read_pairs4(rng, ref, N_PAIRS, 150, mix, dists=dists, noise=0.10)
    f1, f2 = os.path.join(tmp, name + "_1.fq"), os.path.join(tmp, name + "_2.fq")
    reflib.write_fastq(f1, reads[0::2], name)
    reflib.write_fastq(f2, reads[1::2], name)
    ref_sam = _run(fa, [f1, f2], os.path.join(tmp, name + "_ref.sam"), EXTRA, False)
    assert len(ref_sam) >= 2 * N_PAIRS
    return tmp, fa, [f1, f2], ref_sam, _run.last_stderr


@pytest.fixture(scope="module")
def four(genome):  # noqa: F811
    """the four-orientation library and the reference's SAM, made once for both settings"""
    lib = _library(genome, "o4", og.MIXES["all4"], og.READ_DISTS)
    ref_sam, ref_err = lib[3], lib[4]
    assert len(re.findall(r"analyzing insert size distribution for orientation", ref_err)) >= 3, ref_err[-2000:]
    n = proper_pairs_by_orientation(ref_sam)
    print("properly paired, read 1:", dict(zip(og.NAMES, n)))
    assert sum(n[d] >= 50 for d in (og.FF, og.RF, og.RR)) >= 2, n
    return lib


def _device_lines(err, n_pairs):
    """every pair decided on the device without a fall-back, rescue without a host de-duplication, phase 1 from the device"""
    assert _shim_line(err) == (n_pairs, 0)
    d = re.findall(r"mate rescue on the device: (\d+) active pairs, (\d+) host dedup callbacks", err)
    assert d and sum(int(x[0]) for x in d) >= 100 and all(int(x[1]) == 0 for x in d), d
    assert _from_device(err)[0] >= n_pairs
    assert _dedup_line(err)[2] == 0


@pytest.mark.parametrize("more", [None, EVERY_DEVICE], ids=["host_paths", "every_device_switch"])
def test_four_orientation_library_sam_identical(four, more):
    tmp, fa, fqs, ref_sam, _ = four
    dut_sam = _run(fa, fqs, os.path.join(tmp, "o4_dut.sam"), EXTRA, True, more)
    assert ref_sam == dut_sam
    m = re.findall(r"mate rescue: (\d+) pairs, (\d+) ksw_align2 calls in (\d+) GPU rounds", _run.last_stderr)
    assert m and sum(int(x[1]) for x in m) > 1000
    if more:
        _device_lines(_run.last_stderr, N_PAIRS)


def test_mate_pair_library_sam_identical_with_every_device_switch(genome):  # noqa: F811
    dists = tuple((2500, 150) if d == og.RF else x for d, x in enumerate(og.READ_DISTS))
    tmp, fa, fqs, ref_sam, ref_err = _library(genome, "rf", (0, 0, 1, 0), dists)
    assert re.findall(r"analyzing insert size distribution for orientation (..)", ref_err) == ["RF"], ref_err[-2000:]
    n = proper_pairs_by_orientation(ref_sam)
    assert n[og.RF] >= N_PAIRS // 2 and n[og.FR] == 0, n
    dut_sam = _run(fa, fqs, os.path.join(tmp, "rf_dut.sam"), EXTRA, True, EVERY_DEVICE)
    assert ref_sam == dut_sam
    _device_lines(_run.last_stderr, N_PAIRS)
