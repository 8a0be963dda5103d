"""bmh_region_cigar_batch_long -- a region record of any CIGAR and MD length, the flagged regions finished on the device behind the
others (csrc/region_long.hip) -- on the regions of tests/regionlonggen.py: field by field and word by word against the oracle's
ksw_global2 on oriented copies made in numpy, the band loop replayed in Python and a restatement of bwa.c:134-164 (the generator's
cached reference, which tests/test_region_long_cpu.py ties to orc_reg2cigar).  Then the batch shapes around the kernels' blocks,
the guard bytes, the refusal without a reference, and the switch behind bmh_reg2cigar_batch and the device forms of pass B."""
import numpy as np
import pytest

import kswlib
import regionlonggen as gen
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def params():
    return kswlib.make_params()


@pytest.fixture(scope="module")
def ctx(pkg, params):
    c = pkg.Context(0, params)
    c.set_pac(gen.genome()[1], gen.L_PAC)
    yield c
    c.close()


def _kinds(*names):
    return [i for i, r in enumerate(gen.regions()) if r["kind"] in names]


def _flagged(params, idxs, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP):
    """from the oracle alone: which of the regions idxs outgrow the slots"""
    return [len(gen.reference(params, i)["words"]) > cig_cap or len(gen.reference(params, i)["md"]) > md_cap for i in idxs]


def _check(pkg, params, idxs, out, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP):
    """every region of the batch against the reference: the record, and CIGAR and MD where they must lie"""
    res, cig, md, longs, lcig, lmd = out
    flagged = _flagged(params, idxs, cig_cap, md_cap)
    assert len(res) == len(idxs) and len(longs) == sum(flagged)
    assert np.array_equal(longs["region"], np.flatnonzero(flagged))  # ascending by region, one per flagged record
    at = {int(g["region"]): g for g in longs}
    w_at = m_at = 0
    for j, i in enumerate(idxs):
        x, r = gen.reference(params, i), res[j]
        n, m = len(x["words"]), len(x["md"])
        got = (int(r["score"]), int(r["n_cigar"]), int(r["tries"]), int(r["NM"]), int(r["md_len"]))
        assert got == (x["score"], n, x["tries"], x["NM"], m), (j, i, gen.regions()[i]["kind"], got, (x["score"], n, x["tries"], x["NM"], m))
        if not flagged[j]:
            assert int(r["flags"]) == 0
            assert np.array_equal(cig[j, :n], x["words"]) and bytes(md[j, :m]) == x["md"], (j, i)
            continue
        # the bit or bits bmh_region_cigar_batch would have set (it stops at a cut CIGAR), and BMH_REGION_LONG
        cut = pkg.BMH_REGION_CIGAR_CUT if n > cig_cap else pkg.BMH_REGION_MD_CUT
        assert int(r["flags"]) == cut | pkg.BMH_REGION_LONG, (j, i, r)
        g = at[j]
        assert (int(g["cigar_off"]), int(g["md_off"])) == (w_at, m_at), (j, g, w_at, m_at)  # the pools are dense, in region order
        assert np.array_equal(lcig[w_at:w_at + n], x["words"]), (j, i, gen.regions()[i]["kind"])
        assert bytes(lmd[m_at:m_at + m]) == x["md"], (j, i, gen.regions()[i]["kind"])
        w_at, m_at = w_at + n, m_at + m
    assert (len(lcig), len(lmd)) == (w_at, m_at)


def _long(ctx, params, idxs, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP):
    rpool, ob, reqs, tasks, words = gen.region_batch(params, idxs)
    return ctx.region_cigar_batch_long(rpool, ob, reqs, tasks, words, cig_cap=cig_cap, md_cap=md_cap, guard=64)


def test_every_class_against_the_oracle(pkg, ctx, params):
    """All regions of the generator in one batch: every class of it, the ring kernel's two regions included."""
    c = gen.classes(params)
    gen.check_classes(c)
    idxs = list(range(len(gen.regions())))
    out = _long(ctx, params, idxs)
    _check(pkg, params, idxs, out)
    regions, words, md_bytes, _ = ctx.last_region_long_stats()
    assert (regions, words, md_bytes) == (len(out[3]), len(out[4]), len(out[5])) and regions == len(idxs) - c["unflagged"]


def test_nothing_flagged_equals_the_old_call(pkg, ctx, params):
    idxs = _kinds("short", "short_indel", "short_one")
    assert not any(_flagged(params, idxs))
    rpool, ob, reqs, tasks, words = gen.region_batch(params, idxs)
    res, cig, md, longs, lcig, lmd = ctx.region_cigar_batch_long(rpool, ob, reqs, tasks, words, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP, guard=64)
    r0, c0, m0 = ctx.region_cigar_batch(rpool, ob, reqs, tasks, words, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP)
    assert res.tobytes() == r0.tobytes() and cig.tobytes() == c0.tobytes()
    for j in range(len(idxs)):  # (bytes of an MD slot past md_len: unspecified)
        assert bytes(md[j, :int(res[j]["md_len"])]) == bytes(m0[j, :int(r0[j]["md_len"])])
    assert len(longs) == 0 and len(lcig) == 0 and len(lmd) == 0 and ctx.last_region_long_stats()[:3] == (0, 0, 0)
    _check(pkg, params, idxs, (res, cig, md, longs, lcig, lmd))
    # ... and in a mixed batch the unflagged regions come back exactly as from the old call
    mixed = _kinds("short", "cig25", "md_only")
    rpool, ob, reqs, tasks, words = gen.region_batch(params, mixed)
    res, cig, md, _, _, _ = ctx.region_cigar_batch_long(rpool, ob, reqs, tasks, words, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP)
    r0, c0, m0 = ctx.region_cigar_batch(rpool, ob, reqs, tasks, words, cig_cap=gen.CIG_CAP, md_cap=gen.MD_CAP)
    keep = np.flatnonzero(r0["flags"] == 0)
    assert len(keep) >= 40 and res[keep].tobytes() == r0[keep].tobytes() and cig[keep].tobytes() == c0[keep].tobytes()
    assert all(bytes(md[j, :int(r0[j]["md_len"])]) == bytes(m0[j, :int(r0[j]["md_len"])]) for j in keep)


def test_flagged_first_and_last_of_a_batch(pkg, ctx, params):
    short, cut, mdo = _kinds("short"), _kinds("cig64"), _kinds("md_nogap")
    for idxs in ([cut[0]] + short[:5] + [mdo[0]], [mdo[1]] + short[:5] + [cut[1]], [cut[2]], [mdo[2]], short[:3] + [cut[3]] + short[3:6]):
        _check(pkg, params, idxs, _long(ctx, params, idxs))


@pytest.mark.parametrize("n_flagged", [63, 64, 65])
def test_flagged_counts_around_a_wave(pkg, ctx, params, n_flagged):
    """63, 64 and 65 flagged regions interleaved with unflagged ones (the flagged ones of every kind but the ring's, in turn)"""
    all_idx = list(range(len(gen.regions())))
    fl = [i for i, f in zip(all_idx, _flagged(params, all_idx)) if f and gen.regions()[i]["kind"] != "ring"]
    un = [i for i, f in zip(all_idx, _flagged(params, all_idx)) if not f]
    assert len(fl) >= 65
    idxs = []
    for k in range(n_flagged):
        idxs.append(fl[k])
        idxs += un[(2 * k) % len(un):(2 * k) % len(un) + k % 3]
    out = _long(ctx, params, idxs)
    assert len(out[3]) == n_flagged
    _check(pkg, params, idxs, out)


def test_capacity_one_makes_everything_long(pkg, ctx, params):
    """cig_cap = md_cap = 1: every region is long -- no-gap regions by their MD, with the one word of their CIGAR copied from the slot"""
    idxs = _kinds("short", "short_indel", "md_nogap", "cig25", "try3", "del_first", "del_last", "cig_n")
    out = _long(ctx, params, idxs, cig_cap=1, md_cap=1)
    assert len(out[3]) == len(idxs)
    _check(pkg, params, idxs, out, cig_cap=1, md_cap=1)


def test_no_resident_reference_is_an_argument_error(pkg, params):
    c = pkg.Context(0, params)
    try:
        idxs = _kinds("cig25")
        rpool, ob, reqs, tasks, words = gen.region_batch(params, idxs)
        with pytest.raises(pkg.BmhError) as e:
            c.region_cigar_batch_long(rpool, ob, reqs, tasks, words)
        assert e.value.code == pkg.BMH_E_ARG and "bmh_region_cigar_batch_long needs the resident reference" in str(e.value)
        assert c.last_region_long_stats()[:3] == (-1, -1, -1)
    finally:
        c.close()


# ---- the switch behind bmh_reg2cigar_batch ---------------------------------------------------------------------------------------

def _unpacked(res, cig, md):
    """per region (score, n_cigar, NM, tries, words, MD bytes): what bmh_reg2cigar_batch returns, whatever the offsets"""
    mdb = bytes(md)
    return [(int(r["score"]), int(r["n_cigar"]), int(r["NM"]), int(r["tries"]),
             cig[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].tobytes(),
             mdb[int(r["md_off"]):int(r["md_off"]) + int(r["md_len"]) + 1]) for r in res]


def _on_and_off(c, l_pac, pac, reads, reqs):
    c.set_region_long(False)
    off = _unpacked(*c.reg2cigar_batch(l_pac, pac, reads, reqs))
    st_off = c.last_reg2cigar_stats()
    c.set_region_long(True)
    try:
        on = _unpacked(*c.reg2cigar_batch(l_pac, pac, reads, reqs))
        st_on = c.last_reg2cigar_stats()
    finally:
        c.set_region_long(False)
    assert on == off
    assert st_on[0] == st_off[0] == len(reqs) and st_off[1] == 0 and st_on[2] == 0 and st_on[1] == st_off[2], (st_on, st_off)
    return on, st_on


def test_driver_switch_on_the_generator(pkg, ctx, params):
    idxs = [i for i, r in enumerate(gen.regions()) if r["kind"] != "ring"] + _kinds("ring")
    reads, reqs = gen.cigar_reqs(idxs)
    on, st = _on_and_off(ctx, gen.L_PAC, gen.genome()[1], reads, reqs)
    # the driver's slots: 24 words, 96 bytes
    assert st[1] == sum(_flagged(params, idxs, 24, 96)) > 0
    for j, i in enumerate(idxs):
        x = gen.reference(params, i)
        assert on[j] == (x["score"], len(x["words"]), x["NM"], x["tries"], x["words"].tobytes(), x["md"] + b"\0"), (j, i)


def test_driver_switch_on_the_retry_path_case_and_the_golden_groups(pkg, params):
    """the case of test_golden_gpu.py::test_hip_reg2cigar_long_cigars_take_the_retry_path, and the groups of the fixture"""
    from test_kernel_families_gpu import _ctx_with
    c = _ctx_with({})
    try:
        rng = np.random.default_rng(201)
        l_pac = 20000
        bases = rng.integers(0, 4, l_pac, dtype=np.uint8)
        pad = np.concatenate([bases, np.zeros(4, np.uint8)])
        q4 = pad[: (len(pad) // 4) * 4].reshape(-1, 4)
        pac = (q4[:, 0] << 6 | q4[:, 1] << 4 | q4[:, 2] << 2 | q4[:, 3]).astype(np.uint8)
        c.set_params(params)
        reads, reqs = [], []
        for k in range(60):
            L = int(rng.integers(300, 640))
            pos = int(rng.integers(0, l_pac - L - 50))
            src = bases[pos:pos + L + 40]
            out, i, since = [], 0, 0
            step = 25 if k % 3 else 400  # every third read is an ordinary one
            while len(out) < L and i < len(src):
                since += 1
                if since >= step:
                    since = 0
                    if rng.random() < 0.5:
                        i += 1  # deletion from the read
                    else:
                        out.append(int(rng.integers(0, 4)))  # insertion
                        continue
                out.append(int(src[i]))
                i += 1
            rd = np.array(out[:L], dtype=np.uint8)
            rb, re = pos, pos + i
            rq = np.zeros((), kswlib.CIGAR_REQ)
            if k % 2:  # reverse strand: the read is the reverse complement, the region lies in [l_pac, 2*l_pac)
                rd = (3 - rd[::-1]).astype(np.uint8)
                rb, re = 2 * l_pac - re, 2 * l_pac - rb
            rq["read"], rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"] = len(reads), 0, len(rd), rb, re, len(rd) - 60, 100
            reads.append(rd), reqs.append(rq)
        reqs = np.array(reqs)
        dpac = c.set_pac(pac, l_pac)
        on, st = _on_and_off(c, l_pac, dpac, reads, reqs)
        assert st[1] >= 30 and st[2] == 0, st
        for rq, g in zip(reqs, on):
            oscore, owords, onm, omd, otries = kswlib.orc_reg2cigar(params, l_pac, pac, reads[int(rq["read"])], rq)
            assert g == (oscore, len(owords), onm, otries, owords.tobytes(), omd + b"\0")
        # every group of the fixture.  (Its longest CIGAR has 20 words and its longest MD 88 bytes, clipping included: at the
        # driver's 24 words and 96 bytes no region of it is long, so what the groups pin is that the switch changes nothing there.)
        n_groups = 0
        for p, gl_pac, gpac, greads, greqs, exp in kswlib.golden_cigar_groups():
            c.set_params(p)
            dp = c.set_pac(gpac, gl_pac)
            on, st = _on_and_off(c, gl_pac, dp, greads, greqs)
            past = sum(g[1] > 24 or len(g[5]) - 1 > 96 for g in on)
            assert st[1] == past and st[2] == 0, (st, past)
            n_groups += 1
        assert n_groups == 3
    finally:
        c.close()


# ---- ... and behind the device forms of pass B, which redo the regions past their slots through bmh_reg2cigar_batch -------------

def test_wanted_device_and_phase2_text_device_inherit_the_switch(pkg):
    """the eight regions that outgrow their slots of tests/test_phase2_text_device_gpu.py: the same records, bytes and text with the
    switch on, and every redone region is one the long round finished"""
    import phase2gen as pg
    import test_phase2_text_device_gpu as t2
    whole, c = t2._long_reference(pkg, 60, 20000)
    try:
        reads, vectors, special = t2._outgrowing(whole, np.random.default_rng(61))
        o = pg.opt()
        a = pkg.decide_batch(o, c.idx.l_pac, None, 50, [v.copy() for v in vectors])
        want = [list(k) for k in a["want"]]
        host = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), reads, a["regs"], want, device=False)
        off = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), reads, a["regs"], want, device=True)
        assert c.last_wanted_stats()[2] == 8 and c.last_reg2cigar_stats() == (8, 0, 8)
        seqs = t2._dress(reads, False)
        text_off = c.phase2_text_device(o, c.idx, c.pac, None, 50, seqs, [v.copy() for v in vectors], t2.RG)
        c.set_region_long(True)
        on = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), reads, a["regs"], want, device=True)
        assert c.last_wanted_stats()[2] == 8 and c.last_reg2cigar_stats() == (8, 8, 0)
        for x in (off, on):
            assert x[0].tobytes() == host[0].tobytes()
            cu, mu = int(host[0]["n_cigar"].sum()), int((host[0]["md_len"].astype(np.int64) + 1).sum())
            assert np.array_equal(x[1][:cu], host[1][:cu]) and bytes(x[2][:mu]) == bytes(host[2][:mu])
        text_on = c.phase2_text_device(o, c.idx, c.pac, None, 50, seqs, [v.copy() for v in vectors], t2.RG)
        st = c.last_phase2_text_stats()
        assert st["redone"] == 8 and c.last_reg2cigar_stats() == (8, 8, 0), st
        assert text_on[0] == text_off[0] and np.array_equal(text_on[1], text_off[1])
    finally:
        c.close()
