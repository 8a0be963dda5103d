#!/usr/bin/env python3
"""Generate tests/golden/orient_golden.npz FROM THE REFERENCE ITSELF (oracle/_ref/libbwa_ref.so, build container only): pairing and
mate rescue with all four orientations of mem_infer_dir in play (tests/orientgen.py).

Pairing groups  p<set>_<mix>_: option sets 0 and 2 of postgen.OPTION_SETS x the mixes of orientgen.MIXES (all four open / FR + RF
                only / FF + RR with FR at 5 %), 400 pairs each: the input vectors, the reference's mem_pestat table
                (bwamem_pair.c:46) and its mem_pair (:177) per pair as (score, sub, n_sub, z0, z1), pair k under id 1000 + k as in
                tools/make_postproc_fixture.py -- over the input vectors and (pair_res_marked) over them as mem_sam_pe hands them
                to mem_pair, after mem_mark_primary_se, which may exchange hits of one score.
Rescue groups   r<scoring>v<table>_: byte (130 bp, a = 1) and word (150 bp, a = 2) scoring, each under the table the reference
                infers and under one with all four orientations open over the union of its windows: the genome's pac, the reads,
                the reference's phase-1 regions (mem_align1_core), the table, and the vectors and ksw_align2 counts after the
                reference's own mate rescue (the block of mem_sam_pe at bwamem_pair.c:251-263 over mem_matesw).
The fixture is data; no reference source is stored.  Usage: python tools/make_orient_fixture.py [output path]"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kswgen  # noqa: E402
import kswlib  # noqa: E402
import orientgen as og  # noqa: E402
import postgen  # noqa: E402
import reflib  # noqa: E402

L_PAC = 1_000_000
PAIR_SETS = (0, 2)
N_PAIRS = 400
RESCUE_MIX = (.25, .25, .25, .25)
N_RESCUE = 400


def ref_pairing(L, kw, pairs, l_pac, mark=False):
    """the reference's mem_pestat table and mem_pair rows over flat vectors (2 per pair); mark: as mem_sam_pe calls mem_pair, after
    mem_mark_primary_se (bwamem.c:445) under ids id << 1 | read, which sorts hits of one score by their hash"""
    L.mem_pair.restype = C.c_int
    L.mem_pestat.restype = None
    L.mem_mark_primary_se.restype = None
    L.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    opt = L.mem_opt_init()
    for k, v in kw.items():
        setattr(opt.contents, k, v)
    c_regs = kswlib.regs_to_c(pairs)
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    L.mem_pestat(opt, C.c_int64(l_pac), C.c_int(len(pairs)), c_regs, pes.ctypes.data_as(C.c_void_p))
    pr = np.zeros((len(pairs) // 2, 5), dtype=np.int32)
    for k in range(len(pairs) // 2):
        sub, nsub = C.c_int(0), C.c_int(0)
        z = (C.c_int * 2)(-1, -1)
        for r in range(2 if mark else 0):
            if c_regs[2 * k + r].n:
                L.mem_mark_primary_se(opt, c_regs[2 * k + r].n, c_regs[2 * k + r].a, C.c_int64((1000 + k) << 1 | r))
        o = L.mem_pair(opt, C.c_int64(l_pac), None, pes.ctypes.data_as(C.c_void_p), None, C.byref(c_regs, 2 * k * C.sizeof(kswlib.CAlnregV)),
                       C.c_int(1000 + k), C.byref(sub), C.byref(nsub), z)
        pr[k] = (o, sub.value, nsub.value, z[0], z[1])
    kswlib.regs_from_c(c_regs)
    return pes, pr


def pack_regs(regs):
    return np.concatenate(regs) if sum(len(r) for r in regs) else np.zeros(0, kswlib.ALNREG), np.array([len(r) for r in regs], np.int32)


def open_all(pes):
    t = pes.copy()
    ok = pes["failed"] == 0
    t["failed"] = 0
    t["low"], t["high"] = pes["low"][ok].min(), pes["high"][ok].max()
    return t


def main(path):
    assert reflib.have_ref_bwa()
    L = reflib.lib()
    out, pgroups = {}, []
    for si in PAIR_SETS:
        for mi, (mix_name, mix) in enumerate(og.MIXES.items()):
            rng = np.random.default_rng(20261019 + 10 * si + mi)
            pairs, orient = og.paired_vectors4(rng, N_PAIRS, L_PAC, mix)
            pes, pr = ref_pairing(L, postgen.OPTION_SETS[si], pairs, L_PAC)
            key = f"p{si}_{mix_name}_"
            out[key + "pairs"], out[key + "pairs_n"] = pack_regs(pairs)
            out[key + "orient"], out[key + "pes"], out[key + "pair_res"] = orient, pes, pr
            out[key + "pair_res_marked"] = ref_pairing(L, postgen.OPTION_SETS[si], pairs, L_PAC, mark=True)[1]
            assert (out[key + "pair_res_marked"][:, :3] == pr[:, :3]).all()
            pgroups.append(key)
            won = [0] * 4
            for k in np.nonzero(pr[:, 0] > 0)[0]:
                won[og.infer_dir(L_PAC, int(pairs[2 * k][pr[k, 3]]["rb"]), int(pairs[2 * k + 1][pr[k, 4]]["rb"]))[0]] += 1
            print(key, "open", [og.NAMES[d] for d in range(4) if not pes["failed"][d]], "windows", list(zip(pes["low"].tolist(), pes["high"].tolist())),
                  "won", dict(zip(og.NAMES, won)), "n_sub>0", int((pr[:, 2] > 0).sum()))
    out["pair_groups"], out["pair_l_pac"] = np.array(pgroups), np.int64(L_PAC)

    rng = np.random.default_rng(20261020)
    tmp = tempfile.mkdtemp(prefix="bmh_orient_")
    ref = kswgen.rand_seq(rng, 120000)
    fa = os.path.join(tmp, "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    idx = L.bwa_idx_load(fa.encode(), 7)
    l_pac, pac = reflib.pac_of(idx)
    out["l_pac"], out["pac"] = l_pac, pac
    rgroups = []
    for name, p, length in (("byte", kswlib.make_params(), 130), ("word", kswlib.make_params(a=2, b=5, o_del=8, o_ins=8), 150)):
        opt = reflib.opt_from_params(p)
        opt.contents.b = 5 if name == "word" else 4
        reads, orient = og.read_pairs4(rng, ref, N_RESCUE, length, RESCUE_MIX)
        regs = reflib.ref_align_reads(idx, opt, reads)
        pes_ref = reflib.ref_pestat(idx, opt, regs)
        out[f"r{name}_reads"] = np.concatenate(reads)
        out[f"r{name}_read_len"] = np.array([len(r) for r in reads], np.int32)
        out[f"r{name}_regs"], out[f"r{name}_regs_n"] = pack_regs(regs)
        out[f"r{name}_orient"], out[f"r{name}_params"] = orient, np.array(p)
        o = np.zeros((), kswlib.MATESW_OPT)
        o["pen_unpaired"], o["max_matesw"], o["min_seed_len"] = opt.contents.pen_unpaired, opt.contents.max_matesw, opt.contents.min_seed_len
        out[f"r{name}_opt"], out[f"r{name}_mask_level_redun"] = o, np.float32(opt.contents.mask_level_redun)
        for v, pes in enumerate((pes_ref, open_all(pes_ref))):
            exp, ns = reflib.ref_matesw_pairs(idx, opt, pes, reads, regs)
            key = f"r{name}v{v}_"
            out[key + "pes"] = pes
            out[key + "exp"], out[key + "exp_n"] = pack_regs(exp)
            out[key + "n_sw"] = np.array(ns, np.int32)
            rgroups.append(key)
            grew = [0] * 4
            for k in range(len(reads) // 2):
                grew[orient[k]] += len(exp[2 * k]) > len(regs[2 * k]) or len(exp[2 * k + 1]) > len(regs[2 * k + 1])
            print(key, "open", [og.NAMES[d] for d in range(4) if not pes["failed"][d]], "windows", list(zip(pes["low"].tolist(), pes["high"].tolist())),
                  "SW calls", sum(ns), "pairs whose vector grew", dict(zip(og.NAMES, grew)))
    out["rescue_groups"] = np.array(rgroups)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(kswlib.GOLDEN_DIR, "orient_golden.npz"))
