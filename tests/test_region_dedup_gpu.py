"""mem_sort_and_dedup on the device (bmh_sort_dedup_batch, bmh_ctx_set_regs_dedup; region_dedup_kernel in csrc/chain2reg.hip): the
same survivors, record for record and in order, as the reference's own outputs (tests/golden/postproc_golden.npz), as the host routine
bmh_sort_and_dedup (the same text, host/dedup_core.h) and -- where oracle/_ref exists -- as the compiled reference's
mem_sort_and_dedup; alone and behind the chains-to-regions driver."""
import ctypes as C
import os

import numpy as np
import pytest

import kswlib
import postgen
import reflib
from __graft_entry__ import load_package
from test_chain2reg_gpu import _ctx, _host, _reads, _same, _short_reads, world  # noqa: F401  (world: the module-scoped fixture)
from test_chain_gpu import _default_opt, _smem_opt
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

ALNREG = kswlib.ALNREG
MASKS = (0.95, 0.8, 0.0, 1.0)
STATS = ("seeds_extended", "seeds_skipped", "seeds_speculated", "short_sw", "rounds", "ext_tasks")


def _host_dedup(v, mask):
    lib = load_package().lib()
    lib.bmh_sort_and_dedup.restype = C.c_int
    lib.bmh_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]
    a = np.array(v, dtype=ALNREG, copy=True)
    n = lib.bmh_sort_and_dedup(len(a), a.ctypes.data_as(C.c_void_p), C.c_float(mask))
    return a[:n].copy()


def _split(flat, offs):
    return [flat[int(offs[i]): int(offs[i + 1])].copy() for i in range(len(offs) - 1)]


@pytest.fixture(scope="module")
def ctx():
    c = load_package().Context(0)  # neither parameters nor a reference
    yield c
    c.close()


def test_reference_fixture(ctx):
    """The reference's own mem_sort_and_dedup outputs, one call per option set: the insertion-sort path (n <= 16) and the
    quicksort path (n > 16), on vectors full of equal-re ties."""
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "postproc_golden.npz"))
    n_ties = n_long = 0
    for si, kw in enumerate(postgen.OPTION_SETS):
        p = f"s{si}_"
        vecs = _split(g[p + "in"], g[p + "in_off"])
        want = _split(g[p + "ded"], g[p + "ded_off"])
        got = ctx.sort_dedup_batch(vecs, kw.get("mask_level_redun", 0.95))
        assert len(got) == len(want) == 350
        for i, (a, b) in enumerate(zip(got, want)):
            assert len(a) == len(b) and (a == b).all(), f"set {si} read {i}: dedup differs\ndevice={a}\nref={b}"
        n_ties += sum(int(len(v) - len(np.unique(v["re"]))) for v in vecs)
        n_long += sum(len(v) > 16 for v in vecs)
        assert ctx.last_dedup_stats()[:2] == (sum(len(v) for v in vecs), sum(len(v) for v in want))
    assert n_ties > 250 and n_long > 50


def _dense(rng, n, n_loci):
    """n regions over few loci: equal re, equal (score, rb, qb) and chains of redundant overlapping regions are common."""
    a = np.zeros(n, dtype=ALNREG)
    loci = rng.integers(10_000, 5_000_000, size=n_loci)
    for k in range(n):
        rb = int(loci[rng.integers(0, n_loci)]) + int(rng.choice([0, 0, 0, 1, 2, 5, 40]))
        qb = int(rng.choice([0, 0, 0, 10, 30]))
        ln = int(rng.choice([100, 100, 101, 104, 120, 60]))
        a[k]["rb"], a[k]["re"], a[k]["qb"], a[k]["qe"] = rb, rb + ln, qb, qb + ln + int(rng.choice([0, 0, -1, 2]))
        a[k]["score"] = int(rng.choice([ln, ln, ln - 5, 60, 45]))
        a[k]["truesc"], a[k]["w"], a[k]["seedcov"], a[k]["csub"] = a[k]["score"], 100, int(rng.integers(19, ln)), int(rng.choice([0, 20]))
        a[k]["sub_n"] = k  # tells tied records apart
    return a


def _model(v, mask):
    """The routine's loops restated for a vector WITHOUT equal re (the first sort's order is then the only one): what fired, and the
    (score, rb, qb) keys that survive.  The redundancy test in single precision, as the C text has it."""
    a = v[np.argsort(v["re"], kind="stable")]
    m = np.float32(mask)
    rb, re, qb, qe, sc = (a[f].astype(np.int64) for f in ("rb", "re", "qb", "qe", "score"))
    cur = qe.copy()
    ev = {"overlap": 0, "break": 0, "identical": 0}
    for i in range(1, len(a)):
        if rb[i] >= re[i - 1]:
            continue
        j = i - 1
        while j >= 0 and rb[i] < re[j]:
            if cur[j] != qb[j]:
                orr = re[j] - rb[i]
                oq = cur[j] - qb[i] if qb[j] < qb[i] else cur[i] - qb[j]
                mr, mq = min(re[j] - rb[j], re[i] - rb[i]), min(cur[j] - qb[j], cur[i] - qb[i])
                if np.float32(orr) > m * np.float32(mr) and np.float32(oq) > m * np.float32(mq):
                    ev["overlap"] += 1
                    if sc[i] < sc[j]:
                        cur[i] = qb[i]
                        ev["break"] += 1
                        break
                    cur[j] = qb[j]
            j -= 1
    keys = [(int(sc[k]), int(rb[k]), int(qb[k])) for k in range(len(a)) if cur[k] > qb[k]]
    ev["identical"] = len(keys) - len(set(keys))
    return ev, sorted(set(keys))


@pytest.fixture(scope="module")
def generated():
    """The vectors, and per mask the host routine's answer (computed once, shared)."""
    rng = np.random.default_rng(20261017)
    vecs = postgen.region_vectors(rng, 1500, 3_000_000)
    vecs += [_dense(rng, n, max(1, n // 40 + 1)) for n in (2, 3, 16, 17, 18, 41, 300, 2000)]
    vecs += [_dense(rng, n, 3) for n in (17, 41)] + [_dense(rng, int(n), 2) for n in rng.integers(2, 30, size=40)]
    return vecs, {m: [_host_dedup(v, m) for v in vecs] for m in MASKS}


def test_generated_vectors_against_the_host_routine(ctx, generated):
    vecs, want = generated
    cover = {"overlap": 0, "break": 0, "identical": 0}
    for mask in MASKS:
        got = ctx.sort_dedup_batch(vecs, mask)
        for i, (a, b) in enumerate(zip(got, want[mask])):
            assert len(a) == len(b) and a.tobytes() == b.tobytes(), f"mask {mask} vector {i} ({len(vecs[i])} regions): device={a} host={b}"
        # coverage, from the host routine's inputs and outputs: on vectors without equal re the loops are restated above, and the
        # restatement must arrive at the host's survivors before its word on what fired counts
        for v, b in zip(vecs, want[mask]):
            if len(v) < 2 or len(np.unique(v["re"])) != len(v) or len(v) > 100:
                continue
            ev, keys = _model(v, mask)
            assert keys == sorted((int(x["score"]), int(x["rb"]), int(x["qb"])) for x in b), (mask, v, b)
            for k in cover:
                cover[k] += ev[k] > 0
    assert all(n > 0 for n in cover.values()), cover
    assert sum(len(v) > len(b) for v, b in zip(vecs, want[0.95])) > 100
    assert sum(int(len(v) - len(np.unique(v["re"]))) for v in vecs) > 500  # equal-re ties: which record survives is the sort's


def test_generated_vectors_against_the_compiled_reference(generated):
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    R = reflib.lib()
    R.mem_sort_and_dedup.restype = C.c_int
    R.mem_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]
    vecs, want = generated
    ctx = load_package().Context(0)
    for mask in MASKS:
        got = ctx.sort_dedup_batch(vecs, mask)
        for i, v in enumerate(vecs):
            a = v.copy()
            n = R.mem_sort_and_dedup(len(a), a.ctypes.data_as(C.c_void_p), C.c_float(mask)) if len(a) else 0
            assert len(got[i]) == n and got[i].tobytes() == a[:n].tobytes(), f"mask {mask} vector {i}"
    ctx.close()


def test_shapes_idempotence_and_bad_arguments(ctx, generated):
    pkg = load_package()
    lib = pkg.lib()
    vecs, want = generated
    assert ctx.sort_dedup_batch([], 0.95) == []
    assert ctx.last_dedup_stats()[:2] == (0, 0)
    out = ctx.sort_dedup_batch([np.zeros(0, ALNREG)] * 70, 0.95)
    assert len(out) == 70 and all(len(a) == 0 for a in out)
    big = next(i for i, v in enumerate(vecs) if len(v) == 2000)
    alone = ctx.sort_dedup_batch([vecs[big]], 0.95)
    assert alone[0].tobytes() == want[0.95][big].tobytes() and 1 < len(alone[0]) < 2000
    assert ctx.last_dedup_stats()[:2] == (2000, len(alone[0]))
    multi = [i for i, v in enumerate(vecs) if 2 <= len(v) <= 41 and len(want[0.95][i]) < len(v)]
    # 65 reads: the second block has one live lane
    pick = multi[:65]
    got = ctx.sort_dedup_batch([vecs[i] for i in pick], 0.95)
    assert [a.tobytes() for a in got] == [want[0.95][i].tobytes() for i in pick]
    # 64 reads, only lane 63 has more than one region
    single = [v for v in vecs if len(v) == 1][:40] + [np.zeros(0, ALNREG)] * 23
    assert len(single) == 63
    got = ctx.sort_dedup_batch(single + [vecs[multi[0]]], 0.95)
    assert [a.tobytes() for a in got[:63]] == [a.tobytes() for a in single] and got[63].tobytes() == want[0.95][multi[0]].tobytes()
    # idempotence: the output fed back in comes out unchanged -- wherever that holds for the routine itself.  It does not hold everywhere:
    # the redundancy test is asymmetric in which of two records comes first in the re order (orr = q->re - p->rb), the output is in
    # score order, so the second run's introsort meets records of equal re in another order, and at mask_level_redun = 1.0 two such
    # records of different length are redundant in one orientation only (orr > mr iff the longer one comes second).  So: fed back,
    # the device gives what the host routine gives, vector for vector; that is the input unchanged on every vector at 0.95, 0.8 and
    # 0.0 and on all but a handful at 1.0 (host facts, asserted on the host's answers alone).
    for mask in MASKS:
        twice = [_host_dedup(a, mask) for a in want[mask]]
        changed = sum(a.tobytes() != b.tobytes() for a, b in zip(twice, want[mask]))
        assert changed == 0 if mask != 1.0 else changed <= len(vecs) // 100, (mask, changed)
        again = ctx.sort_dedup_batch(want[mask], mask)
        assert [a.tobytes() for a in again] == [a.tobytes() for a in twice], mask
    # bad arguments: BMH_E_ARG, the vectors untouched, and the context serves the next call
    v0 = np.array(vecs[multi[0]], copy=True)
    arr = (pkg._AlnregV * 2)()
    arr[0].n = arr[0].m = len(v0)
    arr[0].a = v0.ctypes.data
    arr[1].n, arr[1].a = 3, None  # n > 0 and a == NULL
    f = C.c_float(0.95)
    assert lib.bmh_sort_dedup_batch(ctx._h, 2, C.cast(arr, C.c_void_p), f) == pkg.BMH_E_ARG
    assert lib.bmh_sort_dedup_batch(ctx._h, -1, C.cast(arr, C.c_void_p), f) == pkg.BMH_E_ARG
    assert lib.bmh_sort_dedup_batch(ctx._h, 1, None, f) == pkg.BMH_E_ARG
    assert lib.bmh_sort_dedup_batch(None, 1, C.cast(arr, C.c_void_p), f) == pkg.BMH_E_ARG
    arr[1].n, arr[1].a = 2 ** 31, v0.ctypes.data  # more than 2^31-1 regions in all; refused before anything is read
    assert lib.bmh_sort_dedup_batch(ctx._h, 2, C.cast(arr, C.c_void_p), f) == pkg.BMH_E_ARG
    assert arr[0].n == len(v0) and v0.tobytes() == vecs[multi[0]].tobytes()
    assert lib.bmh_sort_dedup_batch(ctx._h, 0, None, f) == pkg.BMH_OK
    assert ctx.sort_dedup_batch([vecs[multi[0]]], 0.95)[0].tobytes() == want[0.95][multi[0]].tobytes()


def test_behind_chain2reg_on_the_reference_fixture():
    """The reference's own mem_chain2aln regions, de-duplicated by the host routine, against the device driver with the switch on."""
    ctx = _ctx_with({})
    assert ctx.last_dedup_stats() == (-1, -1, -1.0)
    removed = n_in = 0
    for p, l_pac, pac, reads, chains, exp in kswlib.golden_chain2aln_groups():
        ctx.set_params(p)
        ctx.set_pac(pac, l_pac)
        want = [_host_dedup(a, 0.95) for a in exp]
        removed += sum(len(a) - len(b) for a, b in zip(exp, want))
        n_in += sum(len(a) for a in exp)
        ctx.set_regs_dedup(True, 0.95)
        _same(ctx.chains2regs_device(l_pac, reads, chains, 0), want, "switch on")
        assert ctx.last_dedup_stats()[:2] == (sum(len(a) for a in exp), sum(len(b) for b in want))
        ctx.set_regs_dedup(False, 0.95)
        _same(ctx.chains2regs_device(l_pac, reads, chains, 0), exp, "switch off again")
    ctx.close()
    assert removed >= 10 and n_in >= 2500, (removed, n_in)


def test_behind_chain2reg_on_generated_batches(world):  # noqa: F811
    pkg = load_package()
    p = kswlib.make_params()
    o = _default_opt()
    so = _smem_opt(o)
    l_pac = world["l_pac"]
    ctx = _ctx(world, p)
    reads = _reads(world, 600, 70, 250) + _short_reads(world, 90)
    msl = int(o["min_seed_len"])
    assert msl == 19
    chains = ctx.seed_chain_batch(so, o, l_pac, reads)
    host, _ = _host(ctx, world, reads, chains, msl)
    want = [_host_dedup(a, 0.95) for a in host]
    n_in, n_out = sum(len(a) for a in host), sum(len(a) for a in want)
    assert n_out < n_in  # the batch removes something
    for name, call in (("chains2regs_device", lambda: ctx.chains2regs_device(l_pac, reads, chains, msl)),
                       ("seed_chain_regs_batch", lambda: ctx.seed_chain_regs_batch(so, o, l_pac, reads, msl))):
        ctx.set_regs_dedup(False, 0.95)
        off = call()
        s_off = ctx.driver_stats()
        _same(off, host, f"{name}, switch off")
        ctx.set_regs_dedup(True, 0.95)
        on = call()
        s_on = ctx.driver_stats()
        _same(on, want, f"{name}, switch on")
        assert s_on == s_off, (name, s_on, s_off)
        assert ctx.last_dedup_stats()[:2] == (sum(len(a) for a in off), sum(len(a) for a in on)) == (n_in, n_out)
        assert [a.tobytes() for a in call()] == [a.tobytes() for a in on]  # twice the same bytes
        with pytest.raises(pkg.BmhError) as e:  # a refused call in between leaves the switch as set
            ctx.chains2regs_device(l_pac, reads[:20], chains[:20], -1)
        assert e.value.code == pkg.BMH_E_ARG
        _same(call(), want, f"{name}, after a refused call")
    ctx.set_regs_dedup(True, 0.8)  # the level is the one the switch was set with
    _same(ctx.chains2regs_device(l_pac, reads, chains, msl), [_host_dedup(a, 0.8) for a in host], "mask_level_redun 0.8")
    ctx.close()
