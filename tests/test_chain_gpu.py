"""Seeds to chains on the device (bmh_chain_batch, bmh_seed_chain_batch; csrc/chain.hip): the same chains, seeds and ORDER as the
reference's mem_chain + mem_chain_flt (tests/golden/chain_golden.npz) and as the host chainer bmh_chain_reads over bmh_seed_batch's
tables -- on repeat-rich genomes, where the B-tree of chains splits, equal keys occur and equal weights are sorted."""
import ctypes as C
import os

import numpy as np
import pytest

import kswgen
import kswlib
import reflib
from __graft_entry__ import load_package
from test_chain_cpu import CHAIN_OPT, _ChainV, _Read
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xffffffffffffffff)


def _cut(flat, cnt):
    return np.split(flat, np.cumsum(cnt)[:-1])


def _golden_groups():
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "chain_golden.npz"))
    for p in [str(x) for x in g["groups"]]:
        o = np.zeros((), dtype=CHAIN_OPT)
        for f, v in zip(CHAIN_OPT.names[:6], g[p + "opt"]):
            o[f] = v
        o["mask_level"], o["chain_drop_ratio"] = g[p + "optf"]
        yield p, g, o


def _tables_from_fixture(lib, o, g, p):
    """The fixture's calls / intervals with sa_off and positions in interval order (what bmh_seed_batch would hand over)."""
    reads = [np.ascontiguousarray(r) for r in _cut(g[p + "reads"], g[p + "read_len"])]
    calls, intvs = _cut(g[p + "calls"], g[p + "n_calls"]), _cut(g[p + "intv"], g[p + "n_intv"])
    fi = np.ascontiguousarray(np.concatenate(intvs))
    lib.bmh_chain_sa_keys.restype = C.c_uint64
    sa_off = np.zeros(len(fi) + 1, dtype=np.uint64)
    nk = lib.bmh_chain_sa_keys(o.ctypes.data_as(C.c_void_p), C.c_uint64(len(fi)), fi.ctypes.data_as(C.c_void_p), sa_off.ctypes.data_as(C.c_void_p), None)
    keys = np.zeros(nk + 1, dtype=np.uint64)
    lib.bmh_chain_sa_keys(o.ctypes.data_as(C.c_void_p), C.c_uint64(len(fi)), fi.ctypes.data_as(C.c_void_p), sa_off.ctypes.data_as(C.c_void_p),
                          keys.ctypes.data_as(C.c_void_p))
    sa_k, sa_pos = np.ascontiguousarray(g[p + "sa_k"]), np.ascontiguousarray(g[p + "sa_pos"])
    at = np.searchsorted(sa_k, keys[:nk])
    assert (sa_k[at] == keys[:nk]).all()
    return reads, calls, intvs, _cut(sa_off[:len(fi)], [len(v) for v in intvs]), sa_pos[at]


def test_chain_batch_matches_reference_fixture():
    lib = load_package().lib()
    ctx = _ctx_with({})
    ctx.set_kernel_timing(True)
    total, deep, ties = 0, 0, 0
    for p, g, o in _golden_groups():
        reads, calls, intvs, offs, pos = _tables_from_fixture(lib, o, g, p)
        got = ctx.chain_batch(o, int(g["l_pac"]), reads, calls, intvs, offs, pos)
        st = ctx.chain_stats()
        assert st["reads"] == len(reads) and st["kernel_ms"] >= 0 and st["chains_in"] >= st["chains_out"]
        it = iter(_cut(g[p + "seeds"], g[p + "n_seeds"]) if len(g[p + "n_seeds"]) else [])
        for r, nch in enumerate(g[p + "n_chains"]):
            want = [next(it) for _ in range(int(nch))]
            assert len(got[r]) == len(want), f"{p} read {r}: {len(got[r])} chains, reference {len(want)}"
            for ci, (a, b) in enumerate(zip(got[r], want)):
                assert len(a) == len(b) and (a == b).all(), f"{p} read {r} chain {ci}: ours={a} ref={b}"
            total += len(want)
            deep += len(want) > 15
        assert st["chains_out"] == sum(len(c) for c in got)
        ties += st["equal_keys"]
    ctx.close()
    assert total > 3000 and deep > 30
    assert ties > 0  # look-ups that met an equal key: the B-tree's equal-key order decided these


# ---- fused vs host on a repeat-rich genome indexed by the compiled reference ------------------------------------------------------

def _host_chains(lib, o, l_pac, reads, tables, offs, sa_pos):
    """bmh_chain_reads (host) over bmh_seed_batch's tables -> per read a list of SEED arrays."""
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    n = len(reads)
    c_reads = (_Read * max(n, 1))()
    for k, r in enumerate(reads):
        c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
    calls, intvs = [t[0] for t in tables], [t[1] for t in tables]
    call_off = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint32)
    intv_off = np.concatenate([[0], np.cumsum([len(v) for v in intvs])]).astype(np.uint64)
    fc = np.ascontiguousarray(np.concatenate(calls + [np.zeros(1, kswlib.SMEM_CALL)]))
    fi = np.ascontiguousarray(np.concatenate(intvs + [np.zeros(1, kswlib.SMEM_INTV)]))
    fo = np.ascontiguousarray(np.concatenate(offs + [np.zeros(1, np.uint64)]))
    pos = np.ascontiguousarray(np.concatenate([sa_pos, np.zeros(1, np.uint64)]))
    out = (_ChainV * max(n, 1))()
    lib.bmh_chain_reads.restype = C.c_int
    rc = lib.bmh_chain_reads(o.ctypes.data_as(C.c_void_p), C.c_int64(l_pac), C.c_int(n), C.cast(c_reads, C.c_void_p),
                             call_off.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), intv_off.ctypes.data_as(C.c_void_p),
                             fi.ctypes.data_as(C.c_void_p), fo.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), C.cast(out, C.c_void_p))
    assert rc == 0, rc
    res = []
    for k in range(n):
        chains = []
        for ci in range(out[k].n):
            c = out[k].a[ci]
            sd = np.zeros(c.n, dtype=kswlib.SEED)
            C.memmove(sd.ctypes.data, c.seeds, c.n * kswlib.SEED.itemsize)
            chains.append(sd)
            libc.free(c.seeds)
        if out[k].a:
            libc.free(C.cast(out[k].a, C.c_void_p))
        res.append(chains)
    return res


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for r, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), f"{what}, read {r}: {len(a)} chains against {len(b)}"
        for ci, (x, y) in enumerate(zip(a, b)):
            assert len(x) == len(y) and (x == y).all(), f"{what}, read {r} chain {ci}: {x} against {y}"


def _smem_opt(o):
    so = np.zeros((), dtype=kswlib.SMEM_OPT)
    so["min_seed_len"], so["split_len"], so["split_width"] = o["min_seed_len"], o["split_len"], o["split_width"]
    so["start_width"], so["min_emit_len"] = 1, o["min_seed_len"]
    return so


def _default_opt():
    L = reflib.lib()
    m = L.mem_opt_init().contents
    o = np.zeros((), dtype=CHAIN_OPT)
    o["w"], o["max_chain_gap"], o["min_seed_len"], o["max_occ"] = m.w, m.max_chain_gap, m.min_seed_len, m.max_occ
    o["split_len"], o["split_width"] = int(m.min_seed_len * m.split_factor + .499), m.split_width
    o["mask_level"], o["chain_drop_ratio"] = m.mask_level, m.chain_drop_ratio
    return o


def _opt_sets():
    base = _default_opt()
    few = base.copy()
    few["max_occ"] = 5
    split = base.copy()
    split["split_width"], split["split_len"] = 1, 60
    narrow = base.copy()
    narrow["w"], narrow["max_chain_gap"], narrow["mask_level"], narrow["chain_drop_ratio"] = 10, 150, 0.3, 0.7
    return [("defaults", base), ("max_occ=5", few), ("split_width=1 split_len=60", split), ("narrow w/gap, mask/drop moved", narrow)]


@pytest.fixture(scope="module")
def repeat_genome():
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    import tempfile
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_chain_fixture
    rng = np.random.default_rng(31337)
    ref, fams = make_chain_fixture.build(rng, 400_000)
    tmp = tempfile.mkdtemp(prefix="bmh_chain_gpu_")
    fa = os.path.join(tmp, "ref.fa")
    reflib.write_fasta(fa, "synth", ref)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac = int(idx.contents.bns.contents.l_pac)
    raw = reflib.bwt_arrays(idx)
    reads = []
    for k in range(2600):
        kind = k % 13
        if kind == 0:
            reads.append(np.zeros(0, np.uint8))  # empty
            continue
        if kind == 1:
            reads.append(kswgen.rand_seq(rng, int(rng.integers(1, 19))).astype(np.uint8))  # shorter than min_seed_len
            continue
        Lr = int(rng.integers(100, 251))
        if rng.random() < 0.6:  # a repeat copy, possibly hanging over its edge
            dst, Lf = fams[int(rng.integers(0, len(fams)))][int(rng.integers(0, 6))]
            pos = dst + int(rng.integers(-Lr // 2, max(1, Lf - Lr // 2)))
        else:
            pos = int(rng.integers(0, len(ref) - Lr - 8))
        pos = min(max(pos, 0), len(ref) - Lr - 8)
        r = kswgen.mutate(rng, ref[pos:pos + Lr + 20], float(rng.choice([0.0, 0.02, 0.05])), 0.003, 0.003, 3)[:Lr].copy()
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        if rng.random() < 0.15:  # a run of Ns
            at = int(rng.integers(0, Lr))
            r[at:at + int(rng.integers(1, 15))] = 4
        reads.append(np.ascontiguousarray(r, dtype=np.uint8))
    return l_pac, raw, reads


def _host_reference(ctx, lib, o, l_pac, reads):
    tables, offs, sa_pos = ctx.seed_batch(_smem_opt(o), int(o["max_occ"]), reads)
    return tables, offs, sa_pos, _host_chains(lib, o, l_pac, reads, [t for t in tables], offs, sa_pos)


_FUSED = {}


def test_seed_chain_batch_matches_host_chaining(repeat_genome):
    l_pac, raw, reads = repeat_genome
    lib = load_package().lib()
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    for name, o in _opt_sets():
        tables, offs, sa_pos, want = _host_reference(ctx, lib, o, l_pac, reads)
        assert sum(len(c) for c in want) > 3000, name
        if name == "defaults":  # reads whose chains split the B-tree's root (with max_occ = 5 none can)
            assert sum(len(c) > 15 for c in want) > 5
        got = ctx.seed_chain_batch(_smem_opt(o), o, l_pac, reads)
        _assert_same(got, want, f"fused, {name}")
        _FUSED[name] = got
        # the device chainer over the host's copy of the same tables
        got2 = ctx.chain_batch(o, l_pac, reads, [t[0] for t in tables], [t[1] for t in tables], offs, sa_pos)
        _assert_same(got2, want, f"bmh_chain_batch, {name}")
    ctx.close()


def test_seed_chain_batch_grows_its_capacities(repeat_genome, monkeypatch):
    l_pac, raw, reads = repeat_genome
    lib = load_package().lib()
    monkeypatch.setenv("BMH_CHAIN_INIT_CAP", "16")
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    for name, o in _opt_sets()[:2]:
        want = _FUSED.get(name)
        if want is None:
            monkeypatch.delenv("BMH_CHAIN_INIT_CAP")
            want = _host_reference(ctx, lib, o, l_pac, reads)[3]
            monkeypatch.setenv("BMH_CHAIN_INIT_CAP", "16")
        _assert_same(ctx.seed_chain_batch(_smem_opt(o), o, l_pac, reads), want, f"grown, {name}")
    ctx.close()


def test_edges_and_errors(repeat_genome):
    l_pac, raw, reads = repeat_genome
    pkg = load_package()
    lib = pkg.lib()
    o = _default_opt()
    so = _smem_opt(o)
    bare = _ctx_with({})
    with pytest.raises(pkg.BmhError) as e:  # no index on the device
        bare.seed_chain_batch(so, o, l_pac, reads[:10])
    assert e.value.code == pkg.BMH_E_ARG
    bare.close()
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    assert ctx.seed_chain_batch(so, o, l_pac, []) == []
    assert ctx.chain_batch(o, l_pac, [], [], [], [], np.zeros(0, np.uint64)) == []
    short = [np.zeros(0, np.uint8)] + [kswgen.rand_seq(np.random.default_rng(k), 5 + k).astype(np.uint8) for k in range(12)]
    assert ctx.seed_chain_batch(so, o, l_pac, short) == [[] for _ in short]
    bad = so.copy()
    bad["min_emit_len"] = int(o["min_seed_len"]) + 1
    mism = [bad]
    for f, d in (("min_seed_len", 1), ("split_len", 3), ("split_width", 1)):
        x = so.copy()
        x[f] = int(x[f]) + d
        mism.append(x)
    for x in mism:
        with pytest.raises(pkg.BmhError) as e:
            ctx.seed_chain_batch(x, o, l_pac, reads[:50])
        assert e.value.code == pkg.BMH_E_ARG
    # a re-seeding record out of smem_next2's order
    batch = reads[:400]
    tables, offs, sa_pos, want = _host_reference(ctx, lib, o, l_pac, batch)
    calls = [t[0].copy() for t in tables]
    r = next(k for k, c in enumerate(calls) if (c["min_intv"] > 1).any())
    k = int(np.nonzero(calls[r]["min_intv"] > 1)[0][0])
    calls[r]["x"][k] += 1
    with pytest.raises(pkg.BmhError) as e:
        ctx.chain_batch(o, l_pac, batch, calls, [t[1] for t in tables], offs, sa_pos)
    assert e.value.code == pkg.BMH_E_ARG
    # an interval that should have positions but has none
    offs2 = [x.copy() for x in offs]
    r2 = next(k for k, x in enumerate(offs2) if (x != NONE).any())
    offs2[r2][np.nonzero(offs2[r2] != NONE)[0][0]] = NONE
    with pytest.raises(pkg.BmhError) as e:
        ctx.chain_batch(o, l_pac, batch, [t[0] for t in tables], [t[1] for t in tables], offs2, sa_pos)
    assert e.value.code == pkg.BMH_E_ARG
    # ... and the same context goes on cleanly
    _assert_same(ctx.chain_batch(o, l_pac, batch, [t[0] for t in tables], [t[1] for t in tables], offs, sa_pos), want, "after the errors")
    _assert_same(ctx.seed_chain_batch(so, o, l_pac, batch), want, "fused, after the errors")
    ctx.close()
