#!/usr/bin/env python3
"""Rates of the long-query Smith-Waterman kernel (sw_long.hip, bmh_ctx_set_wide_sw) against sw_generic_kernel (the switch off) on
mate-rescue shapes (informational; bench.py is the contract metric).

Shapes: word-mode ksw_align2 tasks as mem_matesw builds them (KSW_XSUBO | KSW_XSTART | 19*a) at -A 1, a mate of L bases against a
window of L + 1 000 bases holding a mutated copy.  --shapes L:N,... (default 1000:64,1000:1000,1000:16000,5000:64,5000:1000,
10000:64,10000:1000).  Each shape runs once per side after one warm-up launch (--steps more launches if given); the time is the
Smith-Waterman launch's own (bmh_last_kernel_ms), cells = sum of qlen * tlen of the first pass.  Prints one JSON line per shape.
--sam adds a paired-end `bwa mem` run of long mates with unseedable second mates (mate rescue on every pair): REF (the compiled
reference) against DUT (the preload shim with BMH_WIDE_EXT=1), wall time of each and whether the SAM is identical (minus @PG).
Usage: python tools/sw_long_bench.py [--shapes 5000:1000] [--sides on,off] [--sam] [--sam-scoring "-A 4"]
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
import widesw as ws  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def shape(L, n, distinct=64):
    """n tasks over `distinct` generated (mate, window) pairs (the records share pool bytes: generation stays cheap)."""
    rng = np.random.default_rng(L * 7 + n)
    p = kswlib.make_params(a=1)
    pb = kswgen.PoolBuilder(kswlib.SW_TASK)
    for _ in range(min(n, distinct)):
        q = kswgen.rand_seq(rng, L)
        cp = q.copy()
        hit = rng.random(L) < 0.01
        cp[hit] = (cp[hit] + rng.integers(1, 4, size=int(hit.sum()))) & 3
        lead = int(rng.integers(0, 1000))
        t = np.concatenate([kswgen.rand_seq(rng, lead), cp, kswgen.rand_seq(rng, 1000 - lead)])
        ws.add_task(pb, rng, q, t, ws.matesw_xtra(p))
    pool, base = pb.finish()
    return p, pool, base[np.arange(n) % len(base)].copy()


def measure(L, n, side, steps):
    pkg = load_package()
    p, pool, tasks = shape(L, n)
    ctx = pkg.Context(0, p)
    ctx.set_wide_sw(side == "on")
    ctx.sw_batch(pool, tasks)  # warm-up: workspaces grow here
    ctx.set_kernel_timing(True)
    ms = []
    for _ in range(max(steps, 1)):
        t0 = time.perf_counter()
        ctx.sw_batch(pool, tasks)
        wall = time.perf_counter() - t0
        ms.append(ctx.last_kernel_ms())
    n_long, long_ms = ctx.sw_wide_stats()
    ctx.close()
    cells = int((tasks["qlen"].astype(np.int64) * tasks["tlen"].astype(np.int64)).sum())
    k = float(np.median(ms))
    return {"qlen": L, "tasks": n, "side": side, "launch_ms": round(k, 3), "wall_s": round(wall, 4),
            "gcups_first_pass": round(cells / k * 1e-6, 2), "long_kernel_tasks": n_long}


def sam_run(threads, scoring, n_pairs=160, mates=(8000, 8800), frags=(9000, 9900)):
    rng = np.random.default_rng(47)
    tmp = tempfile.mkdtemp(prefix="bmh_longpair_")
    genome = kswgen.rand_seq(rng, 2_000_000)
    fa = os.path.join(tmp, "g.fa")
    reflib.write_fasta(fa, "g", genome)
    reflib.build_index(fa)
    r1, r2 = ws.long_pairs(rng, genome, n_pairs, mates, frags, n_pairs // 2)
    f1, f2 = os.path.join(tmp, "p_1.fq"), os.path.join(tmp, "p_2.fq")
    reflib.write_fastq(f1, r1, "p")
    reflib.write_fastq(f2, r2, "p")
    out, sams = {}, {}
    for who in ("ref", "dut"):
        env = dict(os.environ)
        if who == "dut":
            env.update({"LD_PRELOAD": load_package().DROPIN_PATH, "BMH_WIDE_EXT": "1", "BMH_VERBOSE": "1"})
        path = os.path.join(tmp, f"{who}.sam")
        t0 = time.perf_counter()
        with open(path, "w") as f:
            r = subprocess.run([reflib.REF_BWA, "mem", "-v", "1", "-t", str(threads)] + scoring + [fa, f1, f2], stdout=f,
                               stderr=subprocess.PIPE, env=env, timeout=1200)
        out[f"{who}_s"] = round(time.perf_counter() - t0, 2)
        out[f"{who}_rc"] = r.returncode
        sams[who] = [l for l in open(path) if not l.startswith("@PG")]
        if who == "dut":
            import re
            m = re.findall(r"wide Smith-Waterman so far: (\d+) ksw_align2", r.stderr.decode())
            out["dut_long_kernel_tasks"] = int(m[-1]) if m else -1
    out.update({"pairs": n_pairs, "mates": list(mates), "scoring": " ".join(scoring), "threads": threads,
                "sam_identical": sams["ref"] == sams["dut"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000:64,1000:1000,1000:16000,5000:64,5000:1000,10000:64,10000:1000")
    ap.add_argument("--sides", default="on,off")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--sam", action="store_true")
    ap.add_argument("--sam-scoring", default="-A 4")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    for s in filter(None, a.shapes.split(",")):
        L, n = (int(x) for x in s.split(":"))
        for side in a.sides.split(","):
            print(json.dumps(measure(L, n, side, a.steps)), flush=True)
    if a.sam:
        print(json.dumps(sam_run(a.threads, a.sam_scoring.split())), flush=True)


if __name__ == "__main__":
    main()
