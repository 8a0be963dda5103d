#!/usr/bin/env python3
"""Whole-pipeline DUT/REF timing on the GPU box (informational; bench.py is the contract metric).

REF = the reference `bwa mem` compiled by oracle/Makefile; DUT = the same binary with
libbwamem_hip_dropin.so preloaded (mem_process_seqs entirely on the library: seeding, chaining, extension, mate rescue,
post-processing, SAM text).  Round 1's tool, kept for single-end runs and planted repeats; bench.py's pipeline_baseline and
tools/pipeline_matrix.sh are what the numbers in DESIGN.md come from.
Reads/s are taken from the reference's own per-chunk line
  [M::mem_process_seqs] Processed N reads in X CPU sec, Y real sec      (reference bwamem.c:1320-1321)
which excludes index loading.  SAM equality is checked as well.
Usage: python tools/pipeline_bench.py [--reads 200000] [--genome 4600000] [--threads 16,64]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kswgen  # noqa: E402
import reflib  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def sim_reads_fast(rng, ref, n, L):
    """Vectorised read simulator: 2 % substitutions, 0.25 % 1-bp deletions, 0.25 % 1-bp insertions, 50 % revcomp."""
    M = 24  # spare bases so that deletions never leave the read short
    pos = rng.integers(0, len(ref) - L - M - 8, size=n)
    idx = pos[:, None] + np.arange(L + M)[None, :]
    frag = ref[idx]
    out = np.empty((n, L), dtype=np.uint8)
    for k in range(n):
        f = frag[k]
        u = rng.random(L + M)
        keep = u >= 0.0025                      # deletions
        f = f[keep]
        ins = np.nonzero(rng.random(len(f)) < 0.0025)[0]
        if len(ins):
            f = np.insert(f, ins, rng.integers(0, 4, size=len(ins)))
        f = f[:L].copy()
        sub = rng.random(L) < 0.02
        f[sub] = (f[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
        if rng.random() < 0.5:
            f = (3 - f[::-1])
        out[k] = f
    return out


def sim_pairs_fast(rng, ref, n, L, noisy_frac):
    """Read pairs (FR, insert 250-450); a fraction of second mates carries 12 % substitutions, so that only mate
    rescue (mem_matesw -> ksw_align2) can place most of them."""
    ins = rng.integers(250, 450, size=n)
    pos = rng.integers(0, len(ref) - 520, size=n)
    a = np.empty((n, L), dtype=np.uint8)
    b = np.empty((n, L), dtype=np.uint8)
    for k in range(n):
        f = ref[pos[k]: pos[k] + L].copy()
        sub = rng.random(L) < 0.02
        f[sub] = (f[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
        g = ref[pos[k] + ins[k] - L: pos[k] + ins[k]].copy()
        sub = rng.random(L) < (0.12 if rng.random() < noisy_frac else 0.02)
        g[sub] = (g[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
        a[k], b[k] = f, 3 - g[::-1]
    return a, b


def run(fa, fq, threads, batch, preload, out, ksw_dropin=True, chain_device=False, regs_device=False, dedup_device=False, matesw_device=False,
        decide_device=False, wanted_device=False, phase2_device=False, samtext_device=False, phase2_text_device=False, pestat_device=False,
        reads_sam_device=False, pairs_sam_device=False, more_env=None):
    env = dict(os.environ)
    env.pop("BMH_PESTAT_DEVICE", None)
    env.pop("BMH_CHAIN_DEVICE", None)
    env.pop("BMH_REGS_DEVICE", None)
    env.pop("BMH_DEDUP_DEVICE", None)
    env.pop("BMH_MATESW_DEVICE", None)
    env.pop("BMH_DECIDE_DEVICE", None)
    env.pop("BMH_WANTED_DEVICE", None)
    env.pop("BMH_PHASE2_DEVICE", None)
    env.pop("BMH_SAMTEXT_DEVICE", None)
    env.pop("BMH_PHASE2_TEXT_DEVICE", None)
    env.pop("BMH_READS_SAM_DEVICE", None)
    env.pop("BMH_PAIRS_SAM_DEVICE", None)
    if preload:
        if pairs_sam_device:
            env["BMH_PAIRS_SAM_DEVICE"] = "1"
        if reads_sam_device:
            env["BMH_READS_SAM_DEVICE"] = "1"
        if phase2_text_device:
            env["BMH_PHASE2_TEXT_DEVICE"] = "1"
        if samtext_device:
            env["BMH_SAMTEXT_DEVICE"] = "1"
        if phase2_device:
            env["BMH_PHASE2_DEVICE"] = "1"
        if wanted_device:
            env["BMH_WANTED_DEVICE"] = "1"
        if decide_device:
            env["BMH_DECIDE_DEVICE"] = "1"
        if matesw_device:
            env["BMH_MATESW_DEVICE"] = "1"
        if chain_device:
            env["BMH_CHAIN_DEVICE"] = "1"
        if regs_device or dedup_device or pestat_device:
            env["BMH_REGS_DEVICE"] = "1"
        if dedup_device or pestat_device:
            env["BMH_DEDUP_DEVICE"] = "1"
        if pestat_device:
            env["BMH_PESTAT_DEVICE"] = "1"
        env["LD_PRELOAD"] = load_package().DROPIN_PATH
        env["BMH_KSW_DROPIN"] = "1" if ksw_dropin else "0"
        env["BMH_VERBOSE"] = "1"
        env["BMH_SMEM_TRACE"] = "1"
        if os.environ.get("BMH_DRIVER_TRACE"):
            env["BMH_DRIVER_TRACE"] = "1"
        env.update(more_env or {})
    t0 = time.time()
    with open(out, "w") as f:
        p = subprocess.run([reflib.REF_BWA, "mem", "-t", str(threads), "-b", str(batch), fa] + (fq if isinstance(fq, list) else [fq]), stdout=f,
                           stderr=subprocess.PIPE, env=env, check=True, timeout=3000)
    wall = time.time() - t0
    reads = real = 0
    chunks = []  # (reads, real seconds) of every chunk, in order
    for m in re.finditer(r"Processed (\d+) reads in ([\d.]+) CPU sec, ([\d.]+) real sec", p.stderr.decode()):
        reads += int(m.group(1))
        real += float(m.group(3))
        chunks.append((int(m.group(1)), float(m.group(3))))
    shim = [l for l in p.stderr.decode().splitlines() if l.startswith("[bwamem_hip]")]
    drv = [l for l in shim if "bmh_chain2aln_batch" in l]
    cgr = [l for l in shim if "bmh_reg2cigar_batch" in l and "regions:" in l]
    shim = [l for l in shim if l not in drv and l not in cgr]
    res = {"reads": reads, "shim": shim[:6] + drv[2:8] + cgr[:4] + shim[-8:], "process_seqs_real_s": real, "reads_per_s": reads / real if real else None, "wall_s": wall,
           "chunks": chunks}
    if preload and reads_sam_device:  # which way the chunks went: the session's line, or the shim's word that a paired-end chunk took the other route
        one = [l for l in shim if "in one session so far" in l]
        res["reads_sam_device"] = {"chunks_in_one_session": len(one), "chunks_the_other_way": sum("in one session: off for this chunk" in l for l in shim),
                                   "so_far": one[-1] if one else None}
    if preload and pairs_sam_device:  # likewise; the chunk lines carry the route's three spans
        one = [l for l in shim if "paired-end reads to SAM text in one session so far" in l]
        res["pairs_sam_device"] = {"chunks_in_one_session": len(one), "chunks_the_other_way": sum("paired-end reads to SAM text in one session: off for this chunk" in l for l in shim),
                                   "so_far": one[-1] if one else None, "spans": [l for l in shim if "pairs to SAM text in" in l]}
    return res


def make_input(a, tmp):
    """The run's genome, its index and its reads under tmp, from a.genome, a.repeats, a.reads, a.pe and a.noisy: (fasta, fastq or the two
    fastq files, seconds the index took).  The same arguments give the same files."""
    rng = np.random.default_rng(20261007)
    ref = kswgen.rand_seq(rng, a.genome)
    for _ in range(a.repeats):  # multi-copy sequence: seeds with many occurrences, secondary hits, mapQ ties, more rescue
        src, dst, L = int(rng.integers(0, a.genome - 4000)), int(rng.integers(0, a.genome - 4000)), int(rng.integers(200, 3000))
        ref[dst:dst + L] = kswgen.mutate(rng, ref[src:src + L + 40], float(rng.choice([0.0, 0.005, 0.02])), 0.001, 0.001, 2)[:L]
    fa, fq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fq")
    reflib.write_fasta(fa, "synth", ref)
    t0 = time.time()
    reflib.build_index(fa)
    t_index = time.time() - t0
    if a.pe:
        m1, m2 = sim_pairs_fast(rng, ref, a.reads // 2, 150, a.noisy)
        fq2 = os.path.join(tmp, "reads_2.fq")
        reflib.write_fastq(fq, list(m1), "p")
        reflib.write_fastq(fq2, list(m2), "p")
        fq = [fq, fq2]
    else:
        reads = sim_reads_fast(rng, ref, a.reads, 150)
        reflib.write_fastq(fq, list(reads))
    return fa, fq, t_index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--threads", default="16,64")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pe", action="store_true", help="paired-end reads; the DUT then also batches mate rescue on the GPU")
    ap.add_argument("--noisy", type=float, default=0.3, help="--pe: fraction of second mates that need rescue")
    ap.add_argument("--repeats", type=int, default=0, help="plant this many diverged repeats (200-3000 bp) in the genome")
    ap.add_argument("--full", action="store_true", help="also time the per-call ksw_global2 GPU drop-in (slow by design)")
    ap.add_argument("--chain-device", action="store_true", help="DUT chains on the device, fused with seeding (BMH_CHAIN_DEVICE=1)")
    ap.add_argument("--regs-device", action="store_true",
                    help="DUT seeds, chains and turns chains into regions in one device call (BMH_REGS_DEVICE=1)")
    ap.add_argument("--dedup-device", action="store_true",
                    help="... and sorts and de-duplicates the regions there too (BMH_DEDUP_DEVICE=1); implies --regs-device")
    ap.add_argument("--matesw-device", action="store_true",
                    help="--pe: the DUT's mate-rescue driver (planning, folding, de-duplication) runs on the device (BMH_MATESW_DEVICE=1)")
    ap.add_argument("--decide-device", action="store_true",
                    help="the DUT's phase 2 decisions (primary marking, pairing, mapQ) run on the device (BMH_DECIDE_DEVICE=1)")
    ap.add_argument("--wanted-device", action="store_true",
                    help="the DUT's phase 2 alignments (bwa_fix_xref2, bands, region records and tasks) are planned on the device (BMH_WANTED_DEVICE=1)")
    ap.add_argument("--phase2-device", action="store_true",
                    help="the DUT's phase 2 decisions and alignments run as one device session (BMH_PHASE2_DEVICE=1)")
    ap.add_argument("--samtext-device", action="store_true",
                    help="the DUT's phase 2 coordinates and SAM text are made on the device (BMH_SAMTEXT_DEVICE=1)")
    ap.add_argument("--phase2-text-device", action="store_true",
                    help="the DUT's whole phase 2 runs as one device session, only SAM text comes down (BMH_PHASE2_TEXT_DEVICE=1)")
    ap.add_argument("--reads-sam-device", action="store_true",
                    help="single-end reads: every batch of the DUT goes from bases to SAM text in one device session (BMH_READS_SAM_DEVICE=1); "
                         "with --pe the chunks go the way they go without it, and the run says so")
    ap.add_argument("--pairs-sam-device", action="store_true",
                    help="--pe: every batch of the DUT goes from bases to SAM text in one device session, parked on the device at the insert-size "
                         "barrier (BMH_PAIRS_SAM_DEVICE=1); single-end chunks go the way they go without it")
    ap.add_argument("--pestat-device", action="store_true",
                    help="--pe: ... and answers mem_pestat's question per pair there (BMH_PESTAT_DEVICE=1); implies --regs-device --dedup-device")
    a = ap.parse_args()
    a.dedup_device = a.dedup_device or a.pestat_device
    a.regs_device = a.regs_device or a.dedup_device
    tmp = tempfile.mkdtemp(prefix="bmh_pipe_")
    fa, fq, t_index = make_input(a, tmp)

    res = {"genome_bp": a.genome, "repeats": a.repeats, "reads": a.reads, "paired": bool(a.pe), "index_s": t_index, "chain_device": bool(a.chain_device), "regs_device": bool(a.regs_device),
           "dedup_device": bool(a.dedup_device), "matesw_device": bool(a.matesw_device), "decide_device": bool(a.decide_device), "wanted_device": bool(a.wanted_device),
           "phase2_device": bool(a.phase2_device), "samtext_device": bool(a.samtext_device), "phase2_text_device": bool(a.phase2_text_device), "pestat_device": bool(a.pestat_device), "reads_sam_device": bool(a.reads_sam_device),
           "pairs_sam_device": bool(a.pairs_sam_device), "runs": []}
    # one untimed DUT run first: on a fresh box the first process to load the HIP runtime and the library's code objects
    # pays for reading them from disk (seconds), which has nothing to do with the pipeline
    run(fa, fq, 8, a.batch, True, os.path.join(tmp, "warm.sam"), ksw_dropin=False)
    for t in [int(x) for x in a.threads.split(",")]:
        r = run(fa, fq, t, a.batch, False, os.path.join(tmp, "ref.sam"))
        refsam = [l for l in open(os.path.join(tmp, "ref.sam")) if not l.startswith("@PG")]
        d1 = run(fa, fq, t, a.batch, True, os.path.join(tmp, "dut.sam"), ksw_dropin=False, chain_device=a.chain_device, regs_device=a.regs_device,
                 dedup_device=a.dedup_device, matesw_device=a.matesw_device, decide_device=a.decide_device, wanted_device=a.wanted_device,
                 phase2_device=a.phase2_device, samtext_device=a.samtext_device, phase2_text_device=a.phase2_text_device, pestat_device=a.pestat_device,
                 reads_sam_device=a.reads_sam_device, pairs_sam_device=a.pairs_sam_device)
        same1 = refsam == [l for l in open(os.path.join(tmp, "dut.sam")) if not l.startswith("@PG")]
        d2 = None
        if a.full:
            d2 = run(fa, fq, t, a.batch, True, os.path.join(tmp, "dut.sam"), ksw_dropin=True, chain_device=a.chain_device, regs_device=a.regs_device,
                 dedup_device=a.dedup_device, matesw_device=a.matesw_device, decide_device=a.decide_device, wanted_device=a.wanted_device,
                 phase2_device=a.phase2_device, samtext_device=a.samtext_device, phase2_text_device=a.phase2_text_device, pestat_device=a.pestat_device,
                 reads_sam_device=a.reads_sam_device, pairs_sam_device=a.pairs_sam_device)
            d2["sam_identical"] = refsam == [l for l in open(os.path.join(tmp, "dut.sam")) if not l.startswith("@PG")]
        res["runs"].append({"threads": t, "batch": a.batch, "ref": r, "dut_phase1_gpu": d1, "sam_identical": same1,
                            "dut_phase1_gpu_plus_percall_global": d2})
        print(json.dumps(res["runs"][-1]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
