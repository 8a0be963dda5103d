"""Chains to regions on the device (bmh_chains2regs_device, bmh_seed_chain_regs_batch; csrc/chain2reg.hip): the same regions, record
for record and in order, as the reference's mem_chain2aln (tests/golden/chain2aln_golden.npz) and as the host driver
(bmh_chain2aln_batch / bmh_chains2regs_batch, itself pinned by that fixture and the whole-SAM suite) -- on generated batches over a
repeat-rich genome, with and without the short-chain pre-step, at the ends of both strands, with the wide extension, and after
refused calls."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

import kswgen
import kswlib
import reflib
from __graft_entry__ import load_package
from test_chain_gpu import _default_opt, _smem_opt
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

STATS = ("seeds_extended", "seeds_skipped", "seeds_speculated", "short_sw", "rounds", "ext_tasks")


def _same(got, want, what):
    assert len(got) == len(want), what
    for r, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) and a.tobytes() == b.tobytes(), f"{what}, read {r}: device={a} host={b}"


def test_fixture_parity():
    """min_seed_len = 0 on every parameter set of the reference's own record.  pool_bytes: the reads plus the 16 bytes of padding
    the host driver counts too (here there is nothing else: the windows come from the resident reference)."""
    ctx = _ctx_with({})
    nreg = 0
    for p, l_pac, pac, reads, chains, exp in kswlib.golden_chain2aln_groups():
        ctx.set_params(p)
        ctx.set_pac(pac, l_pac)
        got = ctx.chains2regs_device(l_pac, reads, chains, 0)
        for r, (a, b) in enumerate(zip(got, exp)):
            assert len(a) == len(b) and (a == b).all(), f"read {r}: device={a} ref={b}"
            nreg += len(b)
        st = ctx.driver_stats()
        assert 1 <= st["rounds"] <= 2 and st["ext_tasks"] > 0, st
        assert st["seeds_extended"] == sum(len(b) for b in exp) and st["seeds_speculated"] >= 0 and st["short_sw"] == 0, st
        assert st["pool_bytes"] == sum(len(r) for r in reads) + 16, st
    ctx.close()
    assert nreg >= 2500


# ---- generated batches over a repeat-rich genome indexed by the compiled reference ----------------------------------------------

@pytest.fixture(scope="module")
def world():
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_chain_fixture
    rng = np.random.default_rng(20261)
    ref, fams = make_chain_fixture.build(rng, 300_000)
    tmp = tempfile.mkdtemp(prefix="bmh_c2r_gpu_")
    fa = os.path.join(tmp, "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac, pac = reflib.pac_of(idx)
    return {"rng": rng, "ref": np.asarray(ref, dtype=np.uint8), "fams": fams, "l_pac": l_pac, "pac": pac, "raw": reflib.bwt_arrays(idx)}


def _reads(world, n, lo, hi):
    rng, ref, fams = world["rng"], world["ref"], world["fams"]
    out = []
    for k in range(n):
        Lr = int(rng.integers(lo, hi + 1))
        if rng.random() < 0.6:  # a repeat copy, possibly hanging over its edge: many chains per read
            dst, Lf = fams[int(rng.integers(0, len(fams)))][int(rng.integers(0, 6))]
            pos = dst + int(rng.integers(-Lr // 2, max(1, Lf - Lr // 2)))
        else:
            pos = int(rng.integers(0, len(ref) - Lr - 8))
        pos = min(max(pos, 0), len(ref) - Lr - 28)
        r = kswgen.mutate(rng, ref[pos:pos + Lr + 20], float(rng.choice([0.0, 0.02, 0.05])), 0.003, 0.003, 3)[:Lr].copy()
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        if rng.random() < 0.1:
            at = int(rng.integers(0, Lr))
            r[at:at + int(rng.integers(1, 10))] = 4
        out.append(np.ascontiguousarray(r, dtype=np.uint8))
    return out


def _short_reads(world, n):
    """40-90 genome bases between random flanks of 61-80 bases: mem_chain2aln_short's qualifying test accepts their chains.  Every
    third read continues the genome for 30 more bases on either side with a mismatch every 9th base -- no seed there, but the
    Smith-Waterman runs into the flank, so its verdict leaves the chain to mem_chain2aln."""
    rng, ref = world["rng"], world["ref"]
    out = []
    for k in range(n):
        m = int(rng.integers(40, 91))
        f5, f3 = int(rng.integers(61, 81)), int(rng.integers(61, 81))
        pos = int(rng.integers(200, len(ref) - 400))
        a, b = kswgen.rand_seq(rng, f5).astype(np.uint8), kswgen.rand_seq(rng, f3).astype(np.uint8)
        if k % 3 == 0:
            l5, l3 = ref[pos - 30:pos].copy(), ref[pos + m:pos + m + 30].copy()
            l5[::9] = (l5[::9] + 1) & 3
            l3[4::9] = (l3[4::9] + 1) & 3
            a[-30:], b[:30] = l5, l3
        r = np.concatenate([a, ref[pos:pos + m], b]).astype(np.uint8)
        if k % 2:
            r = (3 - r[::-1]).astype(np.uint8)
        out.append(np.ascontiguousarray(r))
    return out


def _ctx(world, p):
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.set_bwt(*world["raw"])
    world["pac_kept"] = ctx.set_pac(world["pac"], world["l_pac"])
    return ctx


def _host(ctx, world, reads, chains, msl):
    pac, l_pac = world["pac_kept"], world["l_pac"]
    regs = ctx.chain2aln_batch(l_pac, pac, reads, chains) if msl == 0 else ctx.chains2regs_batch(l_pac, pac, reads, chains, msl)
    return regs, ctx.driver_stats()


def _compare(ctx, world, reads, chains, msl, what):
    want, hs = _host(ctx, world, reads, chains, msl)
    got = ctx.chains2regs_device(world["l_pac"], reads, chains, msl)
    ds = ctx.driver_stats()
    _same(got, want, what)
    # the request rule is the host's, literally, so the speculation is the same as well
    for f in ("seeds_extended", "seeds_skipped", "seeds_speculated", "short_sw", "rounds"):
        assert ds[f] == hs[f], (what, f, ds, hs)
    assert ds["ext_tasks"] == hs["ext_tasks"], (what, ds, hs)
    return got, ds


SCORING = {"default": {}, "scaled": dict(a=2, b=7, o_del=9, e_del=3, o_ins=11, e_ins=2, zdrop=150, pen_clip5=9, pen_clip3=7)}


@pytest.mark.parametrize("w", [100, 8])
@pytest.mark.parametrize("scoring", ["default", "scaled"])
def test_parity_with_the_host_driver(world, w, scoring):
    p = kswlib.make_params(w=w, **SCORING[scoring])
    o = _default_opt()
    o["w"] = w
    ctx = _ctx(world, p)
    nreg = many = skipped = rounds = 0
    for name, reads in (("150 bp", _reads(world, 900, 150, 150)), ("100-300 bp", _reads(world, 700, 100, 300))):
        chains = ctx.seed_chain_batch(_smem_opt(o), o, world["l_pac"], reads)
        many += sum(len(c) > 4 for c in chains)
        for msl in (0, 19):
            got, st = _compare(ctx, world, reads, chains, msl, f"{name}, w={w}, {scoring}, min_seed_len={msl}")
            nreg += sum(len(a) for a in got)
            skipped, rounds = skipped + st["seeds_skipped"], max(rounds, st["rounds"])
    ctx.close()
    assert nreg > 4000 and many > 100
    assert skipped > 0 and rounds >= 2  # the containment test and a second round took part


def test_short_chains(world):
    p = kswlib.make_params()
    o = _default_opt()
    ctx = _ctx(world, p)
    reads = _short_reads(world, 360) + _reads(world, 100, 150, 150)
    chains = ctx.seed_chain_batch(_smem_opt(o), o, world["l_pac"], reads)
    msl = int(o["min_seed_len"])
    want, hs = _host(ctx, world, reads, chains, msl)
    # the host rule first: the generator alone must meet the bounds
    settled_host = sum(int((a["w"] == 0).sum()) for a in want)  # a settled chain's region has no band (bwamem.c:533-541)
    assert hs["short_sw"] >= 100 and 0 < settled_host < hs["short_sw"], (hs, settled_host)
    got, ds = _compare(ctx, world, reads, chains, msl, "short chains")
    assert ds["short_sw"] >= 100
    settled = sum(int((a["w"] == 0).sum()) for a in got)
    assert settled >= 1 and ds["short_sw"] - settled >= 1, (ds, settled)
    ctx.close()


def test_fused_entry(world):
    p = kswlib.make_params()
    o = _default_opt()
    so = _smem_opt(o)
    ctx = _ctx(world, p)
    reads = _reads(world, 1200, 100, 250) + _short_reads(world, 60) + [np.zeros(0, np.uint8), kswgen.rand_seq(world["rng"], 12).astype(np.uint8)]
    msl = int(o["min_seed_len"])
    chains = ctx.seed_chain_batch(so, o, world["l_pac"], reads)
    cs = ctx.chain_stats()
    want, hs = _host(ctx, world, reads, chains, msl)
    got = ctx.seed_chain_regs_batch(so, o, world["l_pac"], reads, msl)
    ds, cs2 = ctx.driver_stats(), ctx.chain_stats()
    _same(got, want, "fused")
    for f in ("reads", "chains_in", "chains_out", "seeds", "equal_keys"):
        assert cs[f] == cs2[f], (f, cs, cs2)
    for f in ("seeds_extended", "seeds_skipped", "seeds_speculated", "short_sw", "rounds", "ext_tasks"):
        assert ds[f] == hs[f], (f, ds, hs)
    assert ds["pool_bytes"] == 0 and sum(len(a) for a in got) > 1000  # the reads are where seeding put them: nothing uploaded again
    # without the pre-step
    _same(ctx.seed_chain_regs_batch(so, o, world["l_pac"], reads, 0), _host(ctx, world, reads, chains, 0)[0], "fused, min_seed_len=0")
    assert ctx.seed_chain_regs_batch(so, o, world["l_pac"], [], msl) == []
    ctx.close()


def test_both_strands_and_the_ends_of_the_coordinate(world):
    """Reads at the first and last bases of the genome, both strands, with random overhangs: their windows are clamped at 0 and at
    2*l_pac and cut at l_pac (bwamem.c:752-755)."""
    rng, ref, l_pac = world["rng"], world["ref"], world["l_pac"]
    p = kswlib.make_params()
    o = _default_opt()
    ctx = _ctx(world, p)
    reads = []
    for k in range(120):
        L, over = int(rng.integers(100, 200)), int(rng.integers(0, 30))
        at = int(rng.integers(0, 40))
        body = ref[at:at + L] if k % 2 == 0 else ref[len(ref) - at - L:len(ref) - at]
        hang = kswgen.rand_seq(rng, over).astype(np.uint8)
        r = np.concatenate([hang, body]) if k % 2 == 0 else np.concatenate([body, hang])
        r = kswgen.mutate(rng, np.concatenate([r, r[:20]]), 0.02, 0.002, 0.002, 3)[:len(r)].copy()
        if k % 4 >= 2:
            r = (3 - r[::-1]).astype(np.uint8)
        reads.append(np.ascontiguousarray(r, dtype=np.uint8))
    chains = ctx.seed_chain_batch(_smem_opt(o), o, l_pac, reads)
    # every clamp of bwamem.c:750-755 is met by some chain: its window before clamping, from cal_max_gap, leaves the coordinate at 0
    # and at 2*l_pac, and crosses l_pac from either strand
    orc = kswlib.load_oracle()
    pp = np.ascontiguousarray(np.asarray(p, dtype=kswlib.PARAMS).reshape(()))
    gap = lambda q: int(orc.orc_cal_max_gap(pp.ctypes.data_as(C.c_void_p), C.c_int(int(q))))
    hit = {"below 0": 0, "past 2*l_pac": 0, "forward chain past l_pac": 0, "reverse chain below l_pac": 0}
    for rd, chs in zip(reads, chains):
        for sd in chs:
            b = min(int(t["rbeg"]) - (int(t["qbeg"]) + gap(t["qbeg"])) for t in sd)
            e = max(int(t["rbeg"]) + int(t["len"]) + (len(rd) - int(t["qbeg"]) - int(t["len"])) + gap(len(rd) - int(t["qbeg"]) - int(t["len"])) for t in sd)
            fwd = int(sd[0]["rbeg"]) < l_pac
            hit["below 0"] += b < 0
            hit["past 2*l_pac"] += e > 2 * l_pac
            hit["forward chain past l_pac"] += fwd and e > l_pac
            hit["reverse chain below l_pac"] += (not fwd) and b < l_pac
    assert all(v > 0 for v in hit.values()), hit
    for msl in (0, 19):
        got, _ = _compare(ctx, world, reads, chains, msl, f"ends, min_seed_len={msl}")
    want = kswlib.orc_chain2aln_reads(p, l_pac, world["pac"], reads, chains)  # ... and the CPU oracle's mem_chain2aln
    _same(ctx.chains2regs_device(l_pac, reads, chains, 0), want, "ends against the oracle")
    ctx.close()


def test_edge_shapes_errors_and_determinism(world):
    pkg = load_package()
    rng, ref, l_pac = world["rng"], world["ref"], world["l_pac"]
    p = kswlib.make_params()
    o = _default_opt()
    bare = _ctx_with({})
    bare.set_params(p)
    reads = _reads(world, 300, 120, 200)
    ctx = _ctx(world, p)
    chains = ctx.seed_chain_batch(_smem_opt(o), o, l_pac, reads)
    with pytest.raises(pkg.BmhError) as e:  # no resident reference
        bare.chains2regs_device(l_pac, reads[:20], chains[:20], 0)
    assert e.value.code == pkg.BMH_E_ARG and "bmh_ctx_set_pac" in str(e.value)
    bare.close()
    want, _ = _host(ctx, world, reads, chains, 19)
    with pytest.raises(pkg.BmhError) as e:  # regs[r] not empty
        ctx.chains2regs_device(l_pac, reads[:20], chains[:20], 19, regs_in=[np.zeros(0, kswlib.ALNREG)] * 3 + [want[0] if len(want[0]) else np.zeros(1, kswlib.ALNREG)])
    assert e.value.code == pkg.BMH_E_ARG
    with pytest.raises(pkg.BmhError) as e:
        ctx.chains2regs_device(l_pac, reads[:20], chains[:20], -1)
    assert e.value.code == pkg.BMH_E_ARG
    bad = [[x.copy() for x in c] for c in chains[:20]]
    k = next(r for r in range(20) if len(bad[r]))
    bad[k][0]["len"][0] = len(reads[k]) + 1  # a seed that does not lie inside its read: BMH_E_ARG, as the host driver answers
    with pytest.raises(pkg.BmhError) as e:
        ctx.chains2regs_device(l_pac, reads[:20], bad, 19)
    assert e.value.code == pkg.BMH_E_ARG
    ctx.set_params(kswlib.make_params(w=16384))  # 2*w past the fused record's 32767
    with pytest.raises(pkg.BmhError) as e:
        ctx.chains2regs_device(l_pac, reads, chains, 19)
    assert e.value.code == pkg.BMH_E_RANGE
    with pytest.raises(pkg.BmhError) as e:
        ctx.seed_chain_regs_batch(_smem_opt(o), o, l_pac, reads, 19)
    assert e.value.code == pkg.BMH_E_RANGE
    ctx.set_params(p)
    # ... and the same context goes on cleanly; twice the same bytes (append order must not leak)
    a = ctx.chains2regs_device(l_pac, reads, chains, 19)
    b = ctx.chains2regs_device(l_pac, reads, chains, 19)
    _same(a, want, "after the refused calls")
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    f1 = ctx.seed_chain_regs_batch(_smem_opt(o), o, l_pac, reads, 19)
    f2 = ctx.seed_chain_regs_batch(_smem_opt(o), o, l_pac, reads, 19)
    assert [x.tobytes() for x in f1] == [x.tobytes() for x in f2] == [x.tobytes() for x in want]
    # shapes: no reads, one read, a read without chains, an empty chain, a chain of equal-length seeds (the (len, index) tie)
    assert ctx.chains2regs_device(l_pac, [], [], 19) == []
    one = next(r for r in range(len(reads)) if len(chains[r]) >= 2)
    _compare(ctx, world, [reads[one]], [chains[one]], 19, "one read")
    at = 5000
    tie = np.ascontiguousarray(ref[at:at + 160].copy(), dtype=np.uint8)
    tie[[40, 81, 122]] = (tie[[40, 81, 122]] + 1) & 3
    sd = np.zeros(4, dtype=kswlib.SEED)
    for k, q in enumerate((0, 41, 82, 123)):  # four seeds of 37 bases: the reference starts from the last one
        sd[k] = (at + q, q, 37)
    batch = [reads[0], tie, kswgen.rand_seq(rng, 90).astype(np.uint8), reads[1], np.zeros(0, np.uint8)]
    bch = [chains[0], [sd], [], chains[1] + [np.zeros(0, kswlib.SEED)], []]
    for msl in (0, 19):
        got, _ = _compare(ctx, world, batch, bch, msl, f"shapes, min_seed_len={msl}")
        assert len(got[2]) == 0 and len(got[4]) == 0 and len(got[1]) >= 1
    _same(ctx.chains2regs_device(l_pac, batch, bch, 0), kswlib.orc_chain2aln_reads(p, l_pac, world["pac"], batch, bch), "shapes against the oracle")
    ctx.close()


def test_wide_extension(world):
    """Scores past the 16-bit kernels: 400-base reads at a = 100 (l_query * a = 40 000 > 32 000).  Refused without the switch, equal
    to the host driver with it."""
    pkg = load_package()
    p = kswlib.make_params(a=100, b=120, o_del=200, e_del=100, o_ins=200, e_ins=100, zdrop=10000, pen_clip5=500, pen_clip3=500)
    o = _default_opt()
    ctx = _ctx(world, p)
    reads = _reads(world, 200, 400, 400)
    chains = ctx.seed_chain_batch(_smem_opt(o), o, world["l_pac"], reads)
    with pytest.raises(pkg.BmhError) as e:
        ctx.chains2regs_device(world["l_pac"], reads, chains, 0)
    assert e.value.code == pkg.BMH_E_RANGE
    ctx.set_wide_extension(True)
    got, st = _compare(ctx, world, reads, chains, 0, "wide extension")
    assert sum(len(a) for a in got) >= 200 and max(int(a["score"].max()) for a in got if len(a)) > 32000
    ctx.close()
