"""ksw_global2 past the wave kernel's LDS row on the device: bin 4's band-ring kernel bit for bit against the compiled reference
(or the oracle, which test_global_long_cpu.py pins to it) through every entry point that reaches launch_global."""
import numpy as np
import pytest

import globallong as gl
import kswgen
import kswlib
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu


def _want(p, pool, tasks):
    return kswlib.ref_global_batch(p, pool, tasks) if kswlib.have_ref() else kswlib.orc_global_batch(p, pool, tasks)


def _assert_same(want, wcig, res, cig, tasks, what=""):
    bad = gl.check_against(want, wcig, res, cig, tasks)
    assert not bad, f"{what}{len(bad)} differ; first {tasks[bad[0]]}: gpu={res[bad[0]]} want={want[bad[0]]}"


def _ordinary(rng):
    """Tasks of every lane bin (bands up to 63 on 150 bp) and of the wave bin (wide bands, rows past 512)."""
    a = kswgen.gen_glb_realistic(rng, 300, (100, 160))
    b = kswgen.gen_glb_realistic(rng, 40, (600, 3000), hard=True)
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for w in (64, 100, 300):
        q, t = gl.long_pair(rng, int(rng.integers(200, 2000)))
        kswgen._add_glb(pb, q, t, max(w, abs(len(q) - len(t))))
    return gl.concat(a, b, kswgen.finish_glb(pb))


LONG_SPECS = [(10177, 1, "cigar"), (12000, 50, "cigar"), (15000, 200, "tight"), (20000, 800, "cigar"), (24000, 2000, "cigar"),
              (31000, 100, "cigar"), (40000, 30, "tight"), (52000, 200, "cigar"), (65535, 100, "cigar"), (18000, 300, "score"),
              (45000, 1500, "score"), (11000, 100, "short"), (30000, 50, "short"), (14000, 64, "cigar"), (16000, 128, "tight")]


def test_long_regions_match_reference():
    rng = np.random.default_rng(8100)
    for scoring in (dict(), dict(a=2, b=5, o_del=7, e_del=2, o_ins=5, e_ins=1)):
        p = kswlib.make_params(**scoring)
        ctx = _ctx_with({})
        ctx.set_params(p)
        pool, tasks, words = gl.gen_long(rng, LONG_SPECS)
        want, wcig = _want(p, pool, tasks)
        res, cig = ctx.global_batch(pool, tasks, words)
        _assert_same(want, wcig, res, cig, tasks)
        assert ctx.global_long_stats()[0] == gl.long_count(p, tasks) == len(tasks)
        short = tasks["qlen"].astype(int) > tasks["tlen"].astype(int) + tasks["w"]
        assert short.sum() == 2 and (res["score"][short] == -0x40000000).all()
        # the running count adds up over the context's launches
        ctx.global_batch(pool, tasks[:3], words)
        assert ctx.global_long_stats()[0] == len(tasks) + 3
        ctx.close()


def test_long_stats_timing():
    rng = np.random.default_rng(8150)
    p = kswlib.make_params()
    ctx = _ctx_with({})
    ctx.set_params(p)
    pool, tasks, words = gl.gen_long(rng, [(20000, 100, "cigar"), (30000, 100, "score")])
    ctx.set_kernel_timing(True)
    ctx.global_batch(pool, tasks, words)
    n, ms = ctx.global_long_stats()
    assert n == 2 and ms > 0
    ctx.close()


def test_mixed_batch_keeps_ordinary_tasks():
    rng = np.random.default_rng(8200)
    p = kswlib.make_params()
    ctx = _ctx_with({})
    ctx.set_params(p)
    ordi = _ordinary(rng)
    bins = gl.route(p, ordi[1])
    assert {0, 1, 2, 3} <= set(bins.tolist()) and not (bins == 4).any()
    lng = gl.gen_long(rng, [(20000, 100, "cigar"), (41000, 200, "cigar"), (60000, 50, "tight"), (33000, 400, "score")])
    pool, tasks, words = gl.concat(ordi, lng)
    n0 = len(ordi[1])
    base, bcig = ctx.global_batch(ordi[0], ordi[1], ordi[2])
    res, cig = ctx.global_batch(pool, tasks, words)
    assert (res[:n0] == base).all()
    for k, t in enumerate(tasks[:n0]):
        o, n = int(t["cigar_off"]), int(res[k]["n_cigar"])
        assert np.array_equal(cig[o:o + n], bcig[o:o + n])
    want, wcig = _want(p, lng[0], lng[1])
    _assert_same(want, wcig, res[n0:], cig, tasks[n0:])
    assert ctx.global_long_stats()[0] == gl.long_count(p, tasks) == 4
    oc, ocig = kswlib.orc_global_batch(p, ordi[0], ordi[1])
    _assert_same(oc, ocig, base, bcig, ordi[1], "ordinary: ")
    ctx.close()


def test_device_entry_with_large_qcap():
    import torch
    pkg = load_package()
    rng = np.random.default_rng(8300)
    p = kswlib.make_params()  # w = 100: the device path sizes for bands of max(4w, 100) = 400 -> a ring of 1024 slots
    ctx = _ctx_with({})
    ctx.set_params(p)
    dev = torch.device("cuda:0")
    ordi = _ordinary(rng)
    lng = gl.gen_long(rng, [(20000, 100, "cigar"), (39000, 300, "cigar"), (25000, 50, "tight"), (12000, 400, "score"),
                            (30000, 1000, "cigar")])  # the last one's band does not fit the ring
    pool, tasks, words = gl.concat(ordi, lng)
    n0 = len(ordi[1])

    def run():
        d_pool = torch.from_numpy(pool).to(dev)
        d_tasks = torch.from_numpy(tasks.view(np.uint8)).to(dev)
        d_res = torch.zeros(len(tasks) * kswlib.GLB_RES.itemsize, dtype=torch.uint8, device=dev)
        d_cig = torch.zeros(max(words, 1) * 4, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.global_batch_device(d_pool.data_ptr(), d_tasks.data_ptr(), len(tasks), d_res.data_ptr(), d_cig.data_ptr())
        with pytest.raises(pkg.BmhError) as e:
            ctx.sync()
        assert e.value.code == pkg.BMH_E_RANGE
        return d_res.cpu().numpy().view(kswlib.GLB_RES), d_cig.cpu().numpy().view(np.uint32)

    ctx.set_qcap(40000)
    res, cig = run()
    want, wcig = _want(p, lng[0], lng[1][:4])
    _assert_same(want, wcig, res[n0:n0 + 4], cig, tasks[n0:n0 + 4])
    assert res[-1]["score"] == np.iinfo(np.int32).min
    oc, ocig = kswlib.orc_global_batch(p, ordi[0], ordi[1])
    _assert_same(oc, ocig, res[:n0], cig, tasks[:n0], "ordinary: ")
    assert ctx.global_long_stats()[0] == 5
    ctx.close()


def test_sharded_long_tasks_in_both_shards():
    pkg = load_package()
    rng = np.random.default_rng(8400)
    p = kswlib.make_params()
    ctxs = [_ctx_with({}), _ctx_with({})]
    for c in ctxs:
        c.set_params(p)
    a = gl.concat(kswgen.gen_glb_realistic(rng, 100, (100, 150)), gl.gen_long(rng, [(21000, 100, "cigar"), (35000, 200, "score")]))
    b = gl.concat(gl.gen_long(rng, [(15000, 800, "tight"), (50000, 60, "cigar")]), kswgen.gen_glb_realistic(rng, 101, (100, 150)))
    pool, tasks, words = gl.concat(a, b)
    res, cig = pkg.global_batch_sharded(ctxs, pool, tasks, words)
    want, wcig = _want(p, pool, tasks)
    _assert_same(want, wcig, res, cig, tasks)
    per = [c.global_long_stats()[0] for c in ctxs]
    assert sum(per) == 4 and min(per) >= 1, per
    for c in ctxs:
        c.close()


def _pac_of(bases):
    pad = np.concatenate([bases, np.zeros((-len(bases)) % 4 + 4, np.uint8)])
    q4 = pad[: (len(pad) // 4) * 4].reshape(-1, 4)
    return (q4[:, 0] << 6 | q4[:, 1] << 4 | q4[:, 2] << 2 | q4[:, 3]).astype(np.uint8)


@pytest.mark.parametrize("path", ["host copies", "region records"])
def test_reg2cigar_long_regions(path):
    rng = np.random.default_rng(8500)
    l_pac = 300000
    bases = rng.integers(0, 4, l_pac, dtype=np.uint8)
    pac = _pac_of(bases)
    p = kswlib.make_params()
    ctx = _ctx_with({})
    ctx.set_params(p)
    reads, reqs = [], []
    for k, L in enumerate([12000, 15000, 21000, 33000, 47000, 60000, 18000, 26000]):
        pos = int(rng.integers(0, l_pac - L - 2000))
        rd = np.asarray(kswgen.mutate(rng, bases[pos:pos + L], 0.01, 0.003 if k % 3 else 0.0005, 0.003 if k % 3 else 0.0005, 3), np.uint8)
        rb, re = pos, pos + L  # the region spans what the read came from
        if k % 2:  # reverse strand
            rd = (3 - rd[::-1]).astype(np.uint8)
            rb, re = 2 * l_pac - re, 2 * l_pac - rb
        rq = np.zeros((), kswlib.CIGAR_REQ)
        rq["read"], rq["qb"], rq["qe"], rq["rb"], rq["re"] = len(reads), 0, len(rd), rb, re
        rq["truesc"], rq["reg_w"] = len(rd) - int(rng.integers(60, 4 * len(rd) // 100)), int(rng.choice([50, 100, 200]))
        reads.append(rd), reqs.append(rq)
    # ... and ordinary regions beside them
    for k in range(40):
        L = int(rng.integers(100, 300))
        pos = int(rng.integers(0, l_pac - L - 50))
        rd = np.asarray(kswgen.mutate(rng, bases[pos:pos + L], 0.02, 0.005, 0.005, 2), np.uint8)
        rq = np.zeros((), kswlib.CIGAR_REQ)
        rq["read"], rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"] = len(reads), 0, len(rd), pos, pos + L, len(rd) - 30, 100
        reads.append(rd), reqs.append(rq)
    reqs = np.array(reqs)
    if path == "region records":
        pac = ctx.set_pac(pac, l_pac)
    res, cig, md = ctx.reg2cigar_batch(l_pac, pac, reads, reqs)
    mdb = bytes(md)
    big = 0
    for rq, r in zip(reqs, res):
        read = reads[int(rq["read"])]
        oscore, owords, onm, omd, otries = kswlib.orc_reg2cigar(p, l_pac, pac, read, rq)
        words = cig[int(r["cigar_off"]): int(r["cigar_off"]) + int(r["n_cigar"])]
        m = mdb[int(r["md_off"]): int(r["md_off"]) + int(r["md_len"])]
        assert int(r["score"]) == oscore and int(r["tries"]) == otries and int(r["NM"]) == onm, f"req {rq}"
        assert np.array_equal(words, owords)
        assert m == omd.rstrip(b"\0")
        fw, fmd = kswlib.finish_aln(words, m, rq, len(read), l_pac)
        ow, omd2 = kswlib.finish_aln(owords, omd.rstrip(b"\0"), rq, len(read), l_pac)
        assert np.array_equal(fw, ow) and fmd == omd2
        big += len(owords) > 24
    assert big >= 8  # every long region's CIGAR outgrows the small slots
    assert ctx.global_long_stats()[0] >= 8
    ctx.close()
