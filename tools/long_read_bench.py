#!/usr/bin/env python3
"""Rates of the int32 extension kernel (extend_wide.hip, bmh_ctx_set_wide_extension) on long-read shapes (informational; bench.py
is the contract metric).

Shapes, each a flat extension batch on a context with the switch on, timed over --steps launches after --warmup:
  A10_4kb      -A 10 on 4 kb flanks (h0 + qlen*a past 32000: the wide kernel, LDS variant)
  A1_14-40kb   -A 1 on 14-40 kb flanks (past the LDS kernel's 13 632 columns: the wide kernel, LDS or HBM-slab variant)
  inrange      1-3 kb flanks inside the 16-bit domain as they run by default (extend_lds_kernel), and the same batch again in a
               second process under BMH_EXT_MODE=wide (the int32 kernel on the same tasks)
  glb_w100, glb_w200, glb_w800
               flat ksw_global2 batches (bmh_global_batch, with CIGAR) on 12-60 kb regions at w = 100, 200, 800: past the wave
               kernel's 10 176 columns, so every task runs on the band-ring kernel (bin 4)
Cells are band cells, sum of tlen * min(qlen, 2w+1) per task (an upper bound of what the kernels visit).  Prints one JSON line.
--sam [LO-HI] adds a `bwa mem` single-end run on reads of LO-HI bases (default 8500-9500, at --sam-scoring, default "-A 4"):
REF (the compiled reference) against DUT (the preload shim with BMH_WIDE_EXT=1), wall time of each and whether the SAM is
identical (minus @PG).  Reads past 10 kb go through the band-ring kernel in phase 2, e.g. --sam 20000-40000 --sam-scoring "".
--dut-stderr FILE keeps what the shim writes in that run (with BMH_VERBOSE=1 BMH_DRIVER_TRACE=1 in the environment: its counters and
the drivers' trace lines); the shim's own switches, e.g. BMH_REGION_LONG=1, are taken from the environment as well.
Usage: python tools/long_read_bench.py [--steps 5] [--warmup 1] [--shapes A10_4kb,glb_w200,...] [--sam [LO-HI]] [--dut-stderr FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kswgen  # noqa: E402
import kswlib  # noqa: E402
import reflib  # noqa: E402
import widegen as wg  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def shape(name):
    rng = np.random.default_rng(31)
    if name == "A10_4kb":
        p = kswlib.make_params(a=10, b=40, o_del=60, e_del=10, o_ins=60, e_ins=10, zdrop=1000)
        pool, tasks = wg.gen_ext(rng, p, [(int(rng.integers(3900, 4100)), 200) for _ in range(2048)], w=(100,))
    elif name == "A1_14-40kb":
        p = kswlib.make_params(a=1, b=4)
        pool, tasks = wg.gen_ext(rng, p, [(int(rng.integers(14000, 40000)), 200) for _ in range(256)], w=(100,), indel=0.0)
    else:
        p = kswlib.make_params(a=1, b=4)
        pool, tasks = wg.gen_ext(rng, p, [(int(rng.integers(1000, 3000)), 200) for _ in range(4096)], w=(100,))
    return p, pool, tasks


GLB_SHAPES = {"glb_w100": 100, "glb_w200": 200, "glb_w800": 800}


def glb_shape(name):
    import globallong as gl
    rng = np.random.default_rng(37)
    n = 96 if GLB_SHAPES[name] < 800 else 48
    pool, tasks, words = gl.gen_long(rng, [(int(rng.integers(12000, 60000)), GLB_SHAPES[name], "cigar") for _ in range(n)])
    return kswlib.make_params(), pool, tasks, words


def measure_glb(name, steps, warmup):
    pkg = load_package()
    p, pool, tasks, words = glb_shape(name)
    ctx = pkg.Context(0, p)
    for _ in range(warmup):
        ctx.global_batch(pool, tasks, words)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.global_batch(pool, tasks, words)
    dt = (time.perf_counter() - t0) / steps
    ctx.set_kernel_timing(True)
    n0, _ = ctx.global_long_stats()
    ctx.global_batch(pool, tasks, words)
    n1, ms = ctx.global_long_stats()
    ctx.close()
    w = tasks["w"].astype(np.int64)
    cells = int((tasks["tlen"].astype(np.int64) * np.minimum(tasks["qlen"].astype(np.int64), 2 * w + 1)).sum())
    return {"tasks": len(tasks), "ring_tasks": n1 - n0, "s_per_batch": round(dt, 5), "tasks_per_s": round(len(tasks) / dt, 1),
            "band_cells_per_s": round(cells / dt, 1), "ring_kernel_ms": round(ms, 3)}


def measure(name, steps, warmup):
    if name in GLB_SHAPES:
        return measure_glb(name, steps, warmup)
    pkg = load_package()
    p, pool, tasks = shape(name)
    ctx = pkg.Context(0, p)
    ctx.set_wide_extension(True)
    for _ in range(warmup):
        ctx.extend_batch(pool, tasks)
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.extend_batch(pool, tasks)
    dt = (time.perf_counter() - t0) / steps
    ctx.set_kernel_timing(True)
    ctx.extend_batch(pool, tasks)
    wide_n, wide_ms = ctx.extend_wide_stats()
    bins, _ = ctx.extend_bin_ms_sum()
    ctx.close()
    w = np.minimum(tasks["w"].astype(np.int64), 2 ** 15)
    cells = int((tasks["tlen"].astype(np.int64) * np.minimum(tasks["qlen"].astype(np.int64), 2 * w + 1)).sum())
    return {"tasks": len(tasks), "wide_tasks": wide_n, "s_per_batch": round(dt, 5), "tasks_per_s": round(len(tasks) / dt, 1),
            "band_cells_per_s": round(cells / dt, 1), "wide_kernel_ms": round(wide_ms, 3), "lds_kernel_ms": round(bins[5], 3)}


def sam_run(threads, lens=(8500, 9500), scoring=("-A", "4"), n_reads=200, dut_stderr=None):
    rng = np.random.default_rng(43)
    tmp = tempfile.mkdtemp(prefix="bmh_longsam_")
    genome = kswgen.rand_seq(rng, 2_000_000)
    fa = os.path.join(tmp, "g.fa")
    reflib.write_fasta(fa, "g", genome)
    reflib.build_index(fa)
    reads = wg.long_reads(rng, genome, n_reads, lens)
    fq = os.path.join(tmp, "long.fq")
    reflib.write_fastq(fq, reads, "l")
    out = {}
    for who in ("ref", "dut"):
        env = dict(os.environ)
        if who == "dut":
            env.update(LD_PRELOAD=load_package().DROPIN_PATH, BMH_WIDE_EXT="1")
        path = os.path.join(tmp, f"{who}.sam")
        t0 = time.perf_counter()
        with open(path, "w") as f, open(dut_stderr if who == "dut" and dut_stderr else os.devnull, "w") as err:
            subprocess.run([reflib.REF_BWA, "mem", "-v", "1", "-t", str(threads)] + list(scoring) + [fa, fq], stdout=f, stderr=err,
                           env=env, check=True, timeout=1200)
        out[who + "_wall_s"] = round(time.perf_counter() - t0, 3)
        out[who] = [l for l in open(path) if not l.startswith("@PG")]
    same = out.pop("ref") == out.pop("dut")
    return dict(out, reads=len(reads), read_lens=list(lens), scoring=" ".join(scoring), sam_identical=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="A10_4kb,A1_14-40kb,inrange," + ",".join(GLB_SHAPES))
    ap.add_argument("--sam", nargs="?", const="8500-9500", default=None, metavar="LO-HI")
    ap.add_argument("--sam-scoring", default="-A 4")
    ap.add_argument("--sam-reads", type=int, default=200)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dut-stderr", default=None, metavar="FILE",
                    help="keep what the shim writes in the --sam run (BMH_VERBOSE, BMH_DRIVER_TRACE; BMH_REGION_LONG=1 in the environment is the shim's)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one shape in this process (the second process of the in-range comparison)
        print(json.dumps(measure(a.child, a.steps, a.warmup)))
        return
    shapes = [x for x in a.shapes.split(",") if x]
    res = {name: measure(name, a.steps, a.warmup) for name in shapes}
    if "inrange" in shapes:
        env = dict(os.environ, BMH_EXT_MODE="wide", BMH_EXT_SMALL="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "inrange", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           env=env, capture_output=True, text=True, timeout=1200, check=True)
        res["inrange_on_wide_kernel"] = json.loads(r.stdout.strip().splitlines()[-1])
    if a.sam:
        lo, hi = (int(x) for x in a.sam.split("-"))
        res["bwa_mem_long_se"] = sam_run(a.threads, (lo, hi), tuple(a.sam_scoring.split()), a.sam_reads, a.dut_stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
