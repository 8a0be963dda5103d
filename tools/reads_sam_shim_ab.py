#!/usr/bin/env python3
"""Single-end `bwa mem` through the preload shim, route against route, on tools/pipeline_bench.py's input (same-box A/B; informational).

Three settings of the DUT on one FASTQ, every run a fresh process, the settings alternating a, b, c, a, b, c, ...:
  a  the default route
  b  the all-device two-phase route: BMH_REGS_DEVICE=1 BMH_DEDUP_DEVICE=1 BMH_PHASE2_TEXT_DEVICE=1 BMH_REGION_LONG=1
  c  one device session per batch:   BMH_READS_SAM_DEVICE=1 BMH_REGION_LONG=1
With --pe the input is tools/pipeline_bench.py --pe's pairs (three tenths of the second mates need rescue) and the settings are
  a  the default route
  b  the all-device two-phase route: a's b with BMH_MATESW_DEVICE=1 BMH_PESTAT_DEVICE=1
  c  device sessions parked at the insert-size barrier: BMH_PAIRS_SAM_DEVICE=1 BMH_REGION_LONG=1
and the result keeps setting c's last cumulative line and chunk lines (the parked bytes, the three spans).
Before that, with --sweep, setting c under BMH_RS_THREADS = -t, -t + -t/2 and 2 x -t, alternating likewise.
With --parent DIR (a directory that holds another build's libbwamem_hip_dropin.so next to its libbwamem_hip.so), the default route of
that build against this one in alternating pairs.
Reads/s come from the host program's `Processed N reads in X CPU sec, Y real sec` lines: over all chunks, and from the second chunk
on where there is one (--copies K writes the reads K times over, so that `-t 16` sees more than one chunk of 1.07 M reads); the
process wall clock stands beside them.  Every setting's SAM is compared with the reference binary's once.
Usage: python tools/reads_sam_shim_ab.py --reads 400000 --threads 16 [--pe] [--rounds 5] [--sweep] [--copies 6] [--parent DIR] [--out FILE]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pipeline_bench as pb  # noqa: E402

SETTINGS = {"a": {}, "b": {"BMH_REGS_DEVICE": "1", "BMH_DEDUP_DEVICE": "1", "BMH_PHASE2_TEXT_DEVICE": "1", "BMH_REGION_LONG": "1"},
            "c": {"BMH_READS_SAM_DEVICE": "1", "BMH_REGION_LONG": "1"}}
SETTINGS_PE = {"a": {}, "b": dict(SETTINGS["b"], BMH_MATESW_DEVICE="1", BMH_PESTAT_DEVICE="1"), "c": {"BMH_PAIRS_SAM_DEVICE": "1", "BMH_REGION_LONG": "1"}}


def one(fa, fq, threads, batch, out, env):
    r = pb.run(fa, fq, threads, batch, True, out, ksw_dropin=False, more_env=env)
    later = r["chunks"][1:]
    return {"reads_per_s": r["reads_per_s"], "reads_per_s_after_first_chunk": sum(n for n, _ in later) / sum(s for _, s in later) if later else None,
            "wall_s": r["wall_s"], "chunks": len(r["chunks"]), "shim_tail": r["shim"][-3:],
            "session_lines": [l for l in r["shim"] if "to SAM text in" in l][-4:]}


def summary(runs):
    out = {}
    for key in ("reads_per_s", "reads_per_s_after_first_chunk", "wall_s"):
        v = [r[key] for r in runs if r[key] is not None]
        out[key] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} if v else None
    return out


def alternate(names, rounds, fn):
    res = {k: [] for k in names}
    for _ in range(rounds):
        for k in names:
            res[k].append(fn(k))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=400000)
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--copies", type=int, default=1, help="write the reads this many times over (more than one chunk at -t 16 from 3 on)")
    ap.add_argument("--pe", action="store_true", help="paired-end input, and BMH_PAIRS_SAM_DEVICE=1 as setting c")
    ap.add_argument("--sweep", action="store_true", help="first setting c under BMH_RS_THREADS (--pe: BMH_PS_THREADS) = -t, -t + -t/2, 2 x -t")
    ap.add_argument("--parent", help="directory of another build's libbwamem_hip_dropin.so: its default route against this build's")
    ap.add_argument("--out", help="also write the result to this file")
    a = ap.parse_args()
    a.repeats, a.noisy = 0, 0.3 if a.pe else 0.0
    settings, threads_var = (SETTINGS_PE, "BMH_PS_THREADS") if a.pe else (SETTINGS, "BMH_RS_THREADS")
    tmp = tempfile.mkdtemp(prefix="bmh_rs_ab_")
    fa, fq, _ = pb.make_input(a, tmp)
    for one_fq in (fq if isinstance(fq, list) else [fq]) if a.copies > 1 else []:
        body = open(one_fq).read()
        with open(one_fq, "w") as f:
            for _ in range(a.copies):
                f.write(body)
    t, sam = a.threads, os.path.join(tmp, "dut.sam")
    pb.run(fa, fq, 8, a.batch, True, os.path.join(tmp, "warm.sam"), ksw_dropin=False)  # untimed: the first process on a box reads the code objects from disk
    pb.run(fa, fq, t, a.batch, False, os.path.join(tmp, "ref.sam"))
    refsam = [l for l in open(os.path.join(tmp, "ref.sam")) if not l.startswith("@PG")]
    res = {"reads": a.reads * a.copies, "genome_bp": a.genome, "threads": t, "batch": a.batch, "rounds": a.rounds, "paired": bool(a.pe), "settings": settings,
           "sam_identical": {}}
    for k, env in settings.items():
        one(fa, fq, t, a.batch, sam, env)
        res["sam_identical"][k] = refsam == [l for l in open(sam) if not l.startswith("@PG")]
    print(json.dumps({"sam_identical": res["sam_identical"]}), flush=True)
    if a.sweep:
        counts = [t, t + t // 2, 2 * t]
        sw = alternate(counts, a.rounds, lambda n: one(fa, fq, t, a.batch, sam, dict(settings["c"], **{threads_var: str(n)})))
        res["sweep_rs_threads"] = {str(n): summary(v) for n, v in sw.items()}
        print(json.dumps({"sweep_rs_threads": res["sweep_rs_threads"]}), flush=True)
    ab = alternate(list(settings), a.rounds, lambda k: one(fa, fq, t, a.batch, sam, settings[k]))
    res["routes"] = {k: summary(v) for k, v in ab.items()}
    res["routes_last_shim_lines"] = {k: v[-1]["shim_tail"] for k, v in ab.items()}
    res["route_c_session_lines"] = [r["session_lines"] for r in ab["c"]]
    print(json.dumps({"routes": res["routes"]}), flush=True)
    if a.parent:
        libs = {"parent": os.path.join(os.path.abspath(a.parent), "libbwamem_hip_dropin.so"), "this": pb.load_package().DROPIN_PATH}
        assert os.path.exists(libs["parent"]), libs["parent"]
        pa = alternate(["parent", "this"], a.rounds, lambda k: one(fa, fq, t, a.batch, sam, {"LD_PRELOAD": libs[k]}))
        res["default_route_parent_vs_this"] = {k: summary(v) for k, v in pa.items()}
        print(json.dumps({"default_route_parent_vs_this": res["default_route_parent_vs_this"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
