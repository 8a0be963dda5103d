"""Reads to SAM text as two compositions of the package's calls over one context, for tests/test_pipeline_chain_*.py:
  host_chain     the shim's default route (host/interpose.c: align_batch and mem_process_seqs), call for call
  device_chain   the same hand-offs through the device entry points: bmh_seed_chain_regs_batch with the de-duplication and the
                 insert-size words behind it, bmh_matesw_device, bmh_phase2_text_device
Both take a run of tests/golden/pipeline_golden.npz (tools/make_pipeline_fixture.py: the compiled reference's `bwa mem` on a chunk of
reads, with the index arrays, so that nothing of the reference is needed here) and return every hand-off: the regions after phase
1, the insert-size table, the regions after mate rescue, the text."""
import functools
import os
import types

import numpy as np

import kswlib
import mswgen
from __graft_entry__ import load_package
from test_chain_gpu import _host_chains, _smem_opt
from test_pestat_cand_cpu import bits, whole
from test_phase2_text_device_gpu import _sam_batch
from test_postproc_cpu import DEFAULTS, sam_opt
from test_region_dedup_gpu import _host_dedup

RUNS = ("pe0", "se0", "pe1", "se1")
MEM_F_PE = 0x2
ALNREG = kswlib.ALNREG


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "pipeline_golden.npz"))
    return {k: g[k] for k in g.files}


def _cut(flat, lens):
    return [np.ascontiguousarray(x) for x in np.split(flat, np.cumsum(lens)[:-1])] if len(lens) else []


@functools.lru_cache(maxsize=None)
def world():
    """what every run shares: the index arrays (Context.set_bwt's arguments), the packed reference and the contig table"""
    g = fixture()
    contigs = [(int(o), int(n)) for o, n in zip(g["contig_off"], g["contig_len"])]
    return types.SimpleNamespace(raw=(int(g["bwt_primary"]), [int(x) for x in g["bwt_L2"]], int(g["bwt_seq_len"]), g["bwt_words"], int(g["bwt_sa_intv"]), g["bwt_sa"]),
                                 l_pac=int(g["l_pac"]), pac=np.ascontiguousarray(g["pac"], dtype=np.uint8), contigs=contigs,
                                 names=[str(n).encode() for n in g["contig_names"]], genome=g["genome"])


@functools.lru_cache(maxsize=None)
def run(name):
    """One of the fixture's four runs: the reads dressed for phase 2, the option records of every stage (made from the mem_opt_t fields
    the fixture stores, not from a compiled reference) and the reference's SAM body with its per-read offsets."""
    g, key = fixture(), name[:2]
    m = g[name + "_opt"]
    reads = _cut(g[key + "_reads"], g[key + "_read_len"])
    names = [bytes(n) for n in g[key + "_names"].astype("S")]
    quals = [bytes(q) for q in _cut(g[key + "_qual"], g[key + "_read_len"])] if key + "_qual" in g else [None] * len(reads)
    return make_run(name, m, reads, names, quals, bytes(g[name + "_sam"]), g[name + "_sam_off"])


def make_run(name, m, reads, names, quals, sam=None, sam_off=None):
    pkg = load_package()
    co = np.zeros((), dtype=pkg.CHAIN_OPT)  # qa_chain_opt, host/interpose.c
    for f in ("w", "max_chain_gap", "min_seed_len", "max_occ", "split_width", "mask_level", "chain_drop_ratio"):
        co[f] = m[f]
    co["split_len"] = int(int(m["min_seed_len"]) * float(m["split_factor"]) + .499)
    mo = np.zeros((), dtype=kswlib.MATESW_OPT)
    mo["pen_unpaired"], mo["max_matesw"], mo["min_seed_len"] = m["pen_unpaired"], m["max_matesw"], m["min_seed_len"]
    so = sam_opt(**{k: m[k].item() for k in DEFAULTS})
    assert np.array_equal(so["mat"], m["mat"]) and int(so["mapQ_coef_fac"]) == int(m["mapQ_coef_fac"])
    params = kswlib.make_params(**{k: int(m[k]) for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "w", "zdrop", "pen_clip5", "pen_clip3")})
    return types.SimpleNamespace(name=name, pe=bool(int(m["flag"]) & MEM_F_PE), reads=reads, names=names, quals=quals, params=params, chain_opt=co,
                                 smem_opt=_smem_opt(co), sam_opt=so, matesw_opt=mo, level=float(m["mask_level_redun"]), max_occ=int(m["max_occ"]),
                                 min_seed_len=int(m["min_seed_len"]), sam=sam, sam_off=sam_off, mem_opt=m)


def sub_run(r, reads, names, quals):
    """the run's options over other reads (no reference text exists for them)"""
    return make_run(r.name + "-sub", r.mem_opt, reads, names, quals)


def new_context(pkg):
    """a context with the fixture's index, reference, contig offsets and names resident"""
    w = world()
    c = pkg.Context(0)
    c.set_bwt(*w.raw)
    c.pac = c.set_pac(w.pac, w.l_pac)
    c.idx = pkg.make_refidx(w.contigs, w.l_pac, w.names)
    c.set_refidx(c.idx), c.set_refnames(c.idx)
    return c


def slice_bounds(r, k):
    """qa_matesw_slice's and qa_sam_slice's cut of the chunk into k slices of whole pairs (whole reads for single-end)"""
    unit = 2 if r.pe else 1
    nu = len(r.reads) // unit
    return [(unit * (nu * j // k), unit * (nu * (j + 1) // k)) for j in range(k)]


def _hand_offs(**kw):
    return types.SimpleNamespace(**kw)


def host_chain(ctx, r, slices=1):
    """mem_process_seqs of host/interpose.c with every switch off: bmh_seed_batch, bmh_chain_reads, bmh_chains2regs_batch,
    bmh_sort_and_dedup, bmh_pestat, bmh_matesw_batch with the de-duplication callback and
    bmh_sam_batch."""
    pkg, w = load_package(), world()
    lib = pkg.lib()
    ctx.set_params(r.params)
    ctx.set_regs_dedup(False, r.level), ctx.set_pestat_collect(False), ctx.set_regs_drop_exact(False)
    for switch in (ctx.set_decide_device, ctx.set_wanted_device, ctx.set_region_long, ctx.set_phase2_device, ctx.set_samtext_device, ctx.set_phase2_text_device):
        switch(False)  # (the shim sets them per pooled context)
    seeds, sa_off, sa_pos = ctx.seed_batch(r.smem_opt, r.max_occ, r.reads)
    chains = _host_chains(lib, r.chain_opt, w.l_pac, r.reads, seeds, sa_off, sa_pos)
    raw = ctx.chains2regs_batch(w.l_pac, ctx.pac, r.reads, chains, r.min_seed_len)
    regs1 = [_host_dedup(a, r.level) for a in raw]
    pes, cand, regs2, n_sw = None, None, [a.copy() for a in regs1], []
    if r.pe:
        cand = pkg.pestat_candidates(r.sam_opt, w.l_pac, regs1)  # (the words, to compare the device's with)
        pes = whole(lib, r.sam_opt, regs1, w.l_pac)  # bmh_pestat, the shim's default
        cb = mswgen.bmh_dedup_callback(r.level)
        for lo, hi in slice_bounds(r, slices):
            if hi > lo:
                regs2[lo:hi], ns = ctx.matesw_batch(w.l_pac, ctx.pac, r.reads[lo:hi], regs1[lo:hi], pes, r.matesw_opt, cb)
                n_sw += ns
    texts = []
    for lo, hi in slice_bounds(r, slices):
        if hi > lo:
            texts += _sam_batch(pkg, ctx, r.sam_opt, pes, lo, regs2[lo:hi], r.reads[lo:hi], b"", dress=[(r.names[i], None, r.quals[i]) for i in range(lo, hi)])[0]
    text_off = np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64)
    return _hand_offs(raw=raw, regs1=regs1, cand=cand, pes=pes, regs2=regs2, n_sw=n_sw, text=b"".join(texts), text_off=text_off, stats=[])


def device_chain(ctx, r, slices=1):
    """The same hand-offs through the device entry points on the one context."""
    pkg, w = load_package(), world()
    n = len(r.reads)
    ctx.set_params(r.params)
    ctx.set_regs_dedup(True, r.level)
    ctx.set_regs_drop_exact(False)
    ctx.set_pestat_collect(r.pe, r.sam_opt if r.pe else None)
    raw = None
    regs1 = ctx.seed_chain_regs_batch(r.smem_opt, r.chain_opt, w.l_pac, r.reads, r.min_seed_len)
    stats = {"dedup": ctx.last_dedup_stats()[:2], "slices": []}
    pes, cand, regs2, n_sw = None, None, [a.copy() for a in regs1], []
    if r.pe:
        cand = ctx.last_pestat_candidates(n // 2)[0]
        pes = pkg.pestat_from_candidates(r.sam_opt, cand)
        for lo, hi in slice_bounds(r, slices):
            if hi > lo:
                regs2[lo:hi], ns = ctx.matesw_device(w.l_pac, r.reads[lo:hi], regs1[lo:hi], pes, r.matesw_opt, r.level)
                n_sw += ns
    ctx.set_region_long(True), ctx.set_refidx(ctx.idx), ctx.set_refnames(ctx.idx)
    texts, offs = [], [np.zeros(1, dtype=np.int64)]
    for lo, hi in slice_bounds(r, slices):
        if hi <= lo:
            continue
        seqs = [(r.names[i], None, r.reads[i], r.quals[i]) for i in range(lo, hi)]
        text, off = ctx.phase2_text_device(r.sam_opt, ctx.idx, ctx.pac, pes, lo, seqs, regs2[lo:hi], b"")
        st = ctx.last_phase2_text_stats()
        if st["redone"]:  # (the two below are of the last call that had such regions)
            st["reg2cigar"], st["region_long"] = ctx.last_reg2cigar_stats(), ctx.last_region_long_stats()[:3]
        st["n_units"] = (hi - lo) // (2 if r.pe else 1)
        stats["slices"].append(st)
        offs.append(np.asarray(off[1:], dtype=np.int64) + sum(map(len, texts)))
        texts.append(text)
    return _hand_offs(raw=raw, regs1=regs1, cand=cand, pes=pes, regs2=regs2, n_sw=n_sw, text=b"".join(texts), text_off=np.concatenate(offs), stats=stats)


# ---------------------------------------------------------------- comparisons that name the stage, the read and the field

def first_region_difference(got, want):
    """None, or (read, what) for the first read whose vectors differ: a count, or the first record and field of kswlib.ALNREG"""
    if len(got) != len(want):
        return -1, f"{len(got)} vectors against {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if len(a) != len(b):
            return i, f"{len(a)} regions against {len(b)}"
        if a.tobytes() != b.tobytes():
            for k in range(len(a)):
                for f in ALNREG.names:
                    if a[k][f] != b[k][f]:
                        return i, f"region {k}, field {f}: {a[k][f]} against {b[k][f]}"
            return i, "padding bytes"
    return None


def assert_same_hand_offs(dev, host, what):
    """regs1, pes and regs2 of two compositions, in the order of the stages: the message names the first that differs"""
    d = first_region_difference(dev.regs1, host.regs1)
    assert d is None, f"{what}: phase 1 (regs1), read {d[0]}: {d[1]}"
    if host.pes is not None or dev.pes is not None:
        assert np.array_equal(dev.cand, host.cand), f"{what}: insert-size words, pairs {np.flatnonzero(dev.cand != host.cand)[:5]}"
        assert bits(dev.pes) == bits(host.pes), f"{what}: insert-size table (pes): {dev.pes} against {host.pes}"
    d = first_region_difference(dev.regs2, host.regs2)
    assert d is None, f"{what}: mate rescue (regs2), read {d[0]}: {d[1]}"
    assert dev.n_sw == host.n_sw, f"{what}: mate rescue's Smith-Waterman counts"


def assert_text(got, r, what):
    """text and text_off against the reference's SAM body of the run"""
    off = r.sam_off
    assert len(got.text_off) == len(off), (what, len(got.text_off), len(off))
    if got.text != r.sam or not np.array_equal(got.text_off, off):
        for i in range(len(off) - 1):
            a, b = got.text[int(got.text_off[i]):int(got.text_off[i + 1])], r.sam[int(off[i]):int(off[i + 1])]
            assert a == b, f"{what}: SAM text, read {i} ({r.names[i].decode()}):\n got  {a[:600]!r}\n want {b[:600]!r}"
        raise AssertionError(f"{what}: text_off differs at {np.flatnonzero(got.text_off != off)[:5]}")
