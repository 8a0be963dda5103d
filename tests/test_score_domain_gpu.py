"""The DP kernels at the edges of their integer domains, bit for bit against the oracle (which test_score_domain_cpu.py pins to
the reference there): scores at the top of the 16-bit range, gap costs past 2^15 and 2^16, scaled and general matrices, and
tasks on both sides of every routing switch.  Each test asserts, with domaingen's copy of the dispatcher's condition, that its
tasks really sit on both sides of the switch it targets, and each refusal at the limit is followed by an exact batch on the
same context.  The global tests also hold the device's own per-bin task counts (bmh_last_global_bin_counts) to the dispatcher as
glbbin_ref.py restates it: equal results alone do not show which kernel ran."""
import importlib

import numpy as np
import pytest

import devcalls as dc
import domaingen as dg
import glbband_ref as gr
import glbbin_ref as br
import kswgen
import kswlib
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

EXT_ENV = {"auto": {}, "reg": {"BMH_EXT_MODE": "reg", "BMH_EXT_SMALL": "0"}, "grp": {"BMH_EXT_MODE": "grp", "BMH_EXT_SMALL": "0"},
           "lds": {"BMH_EXT_MODE": "lds", "BMH_EXT_SMALL": "0"}, "lanex4": {"BMH_EXT_MODE": "lanex4", "BMH_EXT_SMALL": "0"},
           "lane": {"BMH_EXT_MODE": "lane", "BMH_EXT_SMALL": "0"},
           "persist": {"BMH_EXT_MODE": "lane", "BMH_EXT_SMALL": "0", "BMH_EXT_PERSIST": "1"}}
SEED_ENV = {"auto": {}, "lane": {"BMH_EXT_SMALL": "0"}, "persist": {"BMH_EXT_SMALL": "0", "BMH_EXT_PERSIST": "1"}}
GLB_ENV = {"lane": {}, "own": {"BMH_GLB_NARROW": "0"}, "wave": {"BMH_GLB_MODE": "wave"}, "masked": {"BMH_EXT_SMALL": "0", "BMH_GL_FAST": "0"}}
# what glbbin_ref.expected_bins must be told about each of these contexts; None: no lane kernel runs, everything is in bin 2
GLB_RULE = {"lane": dict(narrow=True), "own": dict(narrow=False), "wave": None, "masked": dict(narrow=True)}
SW_ENV = {"wave": {"BMH_SW_MODE": "default"}, "lane": {"BMH_SW_MODE": "default", "BMH_SW_WAVE": "0"},
          "generic": {"BMH_SW_MODE": "generic"}}
SEED_FIELDS = ("qb", "qe", "rb", "re", "score", "truesc", "w", "n_ext")
EXT_GAPS_MSG = "the extension kernels need o_del+e_del, o_ins+e_ins <= 65535 and e_del, e_ins <= 16383"


def _cmp_ext(ctx, p, pool, tasks, what):
    ctx.set_params(p)
    got = ctx.extend_batch(pool, tasks)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ; first task {tasks[bad[0]]} gpu={got[bad[0]]} oracle={want[bad[0]]}"
    return got


def _cmp_seed(ctx, p, pool, tasks, what):
    ctx.set_params(p)
    got = ctx.seedext_batch(pool, tasks)
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    for f in SEED_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}, {f}: {len(bad)} differ; first seed {tasks[bad[0]]} gpu={got[bad[0]]} oracle={want[bad[0]]}"
    return got


def _cmp_glb(ctx, p, pool, tasks, words, what):
    ctx.set_params(p)
    res, cig = ctx.global_batch(pool, tasks, words)
    ores, ocig = kswlib.orc_global_batch(p, pool, tasks)
    bad = np.nonzero(res != ores)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ; first task {tasks[bad[0]]} gpu={res[bad[0]]} oracle={ores[bad[0]]}"
    for k, (t, r, oc) in enumerate(zip(tasks, res, ocig)):
        o = int(t["cigar_off"])
        assert np.array_equal(cig[o:o + int(r["n_cigar"])], oc), f"{what}: CIGAR of task {k} ({t})"
    return res


def _cmp_sw(ctx, p, pool, tasks, what):
    ctx.set_params(p)
    got = ctx.sw_batch(pool, tasks)
    want, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=8)
    assert (want["rsv"] == 0).all(), "the reference defines every result of these tasks"
    for f in kswlib.SW_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}, {f}: {len(bad)} differ; first task {tasks[bad[0]]} gpu={got[bad[0]]} oracle={want[bad[0]]}"
    return got


# ---- extension ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(EXT_ENV))
def test_extend_at_the_top_of_the_score_range(mode):
    """h0 + qlen*max(mat) of exactly 32000, 31999 and below, queries at every length-bin edge +-1 (extend_dispatch.hip:33),
    bands and end bonuses up to 32767, z-drop -1 / 0 / 30000, and gap costs of 40000 and past 65536 -- which the 16-bit lane
    kernels once read modulo 2^16."""
    pkg = load_package()
    ctx = _ctx_with(EXT_ENV[mode])
    rng = np.random.default_rng(7100)
    top = 0
    sets = dg.ext_edge_param_sets(rng)
    assert sum(not dg.ext_gaps_accepted(p) for p in sets) >= 3 and sum(dg.ext_gaps_accepted(p) for p in sets) >= 6
    for k, p in enumerate(sets):
        pool, tasks = dg.gen_ext_edges(rng, p, per=4, early_indel=int(p["o_del"]) + int(p["e_del"]) > 30000)
        if not dg.ext_gaps_accepted(p):  # o+e past 16 bits or e past 16383: refused; the next batch on the context must be exact
            ctx.set_params(p)
            with pytest.raises(pkg.BmhError) as e:
                ctx.extend_batch(pool, tasks)
            assert e.value.code == pkg.BMH_E_RANGE and EXT_GAPS_MSG in str(e.value)
            continue
        mx = dg.max_mat(p)
        assert ((np.maximum(tasks["h0"], 0) + tasks["qlen"].astype(np.int64) * mx) == dg.LIMIT).any()
        if mx <= 60:  # every bin edge of extend_dispatch.hip:33 is in this batch, on both sides
            bins = {dg.ext_bin(int(q), 4 if mode == "lanex4" else 0) for q in tasks["qlen"]}
            assert {0, 1, 2, 3, 5} <= bins and (mode != "lanex4" or 4 in bins)
        top = max(top, int(_cmp_ext(ctx, p, pool, tasks, f"{mode} set {k}")["score"].max()))
    assert top > 30000
    p = kswlib.make_params(a=3, b=4, o_del=9, e_del=3, o_ins=9, e_ins=3, zdrop=30000)  # the LDS kernel's long queries
    pool, tasks = dg.gen_ext_edges(rng, p, qlens=(255, 257, 10000), per=2, long_q=10666)
    assert dg.ext_bin(10666) == 5 and tasks["qlen"].max() == 10666
    _cmp_ext(ctx, p, pool, tasks, f"{mode} long queries")
    ctx.close()


# ---- fused seed record --------------------------------------------------------------------------------------------------

def _seeds_at(rng, L, n):
    """n seeds on reads of exactly L bases, each read a lightly mutated copy of its window's middle."""
    pool, rows = [], []
    off = 0
    for _ in range(n):
        win = kswgen.rand_seq(rng, L + 200)
        read = win[100:100 + L].copy()
        qbeg, ln = int(rng.integers(0, L - 30)), int(rng.integers(19, 31))
        mask = rng.random(L) < 0.02
        mask[qbeg:qbeg + ln] = False
        read[mask] = (read[mask] + 1) & 3
        pool += [read, win]
        rows.append((off, off + L, L, qbeg, ln, 100 + qbeg, L + 200, 0, 0))
        off += 2 * L + 200
    pool.append(np.zeros(16, np.uint8))
    return np.concatenate(pool).astype(np.uint8), np.array(rows, dtype=kswlib.SEED_TASK)


@pytest.mark.parametrize("mode", list(SEED_ENV))
def test_seedext_at_the_top_of_the_score_range(mode):
    """taskgen's reads under -A 106 -B 127 (300 bp: 31 800) and seeds whose l_query*max(max_mat, a) is exactly 32000 (api.hip:641)."""
    tg = importlib.import_module(load_package().__name__ + ".taskgen")
    ctx = _ctx_with(SEED_ENV[mode])
    rng = np.random.default_rng(7200)
    for kw in (dict(a=106, b=127, o_del=120, e_del=100, o_ins=110, e_ins=106, zdrop=10600, pen_clip5=530, pen_clip3=530),
               dict(a=60, b=127, o_del=65534, e_del=1, o_ins=40000, e_ins=16383, zdrop=6000, pen_clip5=300, pen_clip3=300)):
        p = kswlib.make_params(w=100, **kw)
        pool, tasks = tg.generate_seeds(p, 1500, "mixed100-300", seed=7201)
        assert int(tasks["l_query"].max()) == 300  # 300 * 106 = 31 800
        _cmp_seed(ctx, p, pool, tasks, f"{mode} {kw}")
    p = kswlib.make_params(a=100, b=127, o_del=600, e_del=100, o_ins=600, e_ins=100, zdrop=10000, pen_clip5=500, pen_clip3=500)
    pool, tasks = _seeds_at(rng, 320, 300)
    assert (tasks["l_query"] * 100 == dg.LIMIT).all()
    got = _cmp_seed(ctx, p, pool, tasks, f"{mode} at the limit")
    assert got["score"].max() > 28000
    ctx.close()


# ---- global ---------------------------------------------------------------------------------------------------------------

def _glb_bins(mode, p, pool, tasks):
    """(bin, band run on) of every task under the context of GLB_ENV[mode]."""
    if GLB_RULE[mode] is None:
        return np.full(len(tasks), 2), tasks["w"].astype(np.int64)
    return br.expected_bins(p, pool, tasks, **GLB_RULE[mode])


def _cmp_glb_bins(ctx, mode, p, pool, tasks, words, what):
    """_cmp_glb, and the device's per-bin counts of that launch against the rule's."""
    res = _cmp_glb(ctx, p, pool, tasks, words, what)
    counts, expect = ctx.last_global_bin_counts(), np.bincount(_glb_bins(mode, p, pool, tasks)[0], minlength=8)
    assert (counts == expect).all(), f"{what}: bin counts {counts.tolist()}, the rule gives {expect.tolist()}"
    return res


@pytest.mark.parametrize("mode", list(GLB_ENV))
def test_global_on_both_sides_of_every_switch(mode):
    """global_kernel.hip:273-278 and host/glbbin_core.h: worst 11999 / 12000, o_del+o_ins 3999 / 4000, tlen 512 / 513, w 31/32, 47/48,
    63/64 -- and scores far into the int32 range in the wave kernel's LDS and HBM-scratch variants.  Every batch's per-bin task
    counts on the device are the rule's; on the tasks' own bands ("own") that puts w = 31 on <64>, 32 and 47 on <96>, 48 and 63 on
    <128> and 64 on the wave kernel, and with the band pass ("lane", "masked") wherever the narrowed band says."""
    ctx = _ctx_with(GLB_ENV[mode])
    rng = np.random.default_rng(7300)
    p = kswlib.make_params(a=5, b=20, o_del=30, e_del=1, o_ins=40, e_ins=1)
    pool, tasks, words = dg.gen_glb_worst_edges(rng, p)
    worst = [dg.glb_worst(p, int(t["qlen"]), int(t["tlen"])) for t in tasks]
    assert 11999 in worst and 12000 in worst
    rows_cap = min(int(tasks["tlen"].max()), 512)
    bins = [dg.glb_lane_bin(p, int(t["qlen"]), int(t["tlen"]), int(t["w"]), rows_cap) for t in tasks]
    assert bins[worst.index(12000)] == 2 and bins[worst.index(11999)] != 2
    run = _glb_bins(mode, p, pool, tasks)[0]
    assert ((run == 2) == (np.array(worst) >= 12000)).all() or mode == "wave"  # `worst` alone decides lane or wave here, narrowed or not
    _cmp_glb_bins(ctx, mode, p, pool, tasks, words, f"{mode} worst")

    p = kswlib.make_params()
    pool, tasks, words = dg.gen_glb_shape_edges(rng)
    rows_cap = min(int(tasks["tlen"].max()), 512)
    bins = {(int(t["tlen"]), int(t["w"])): dg.glb_lane_bin(p, int(t["qlen"]), int(t["tlen"]), int(t["w"]), rows_cap) for t in tasks}
    assert rows_cap == 512 and {b for (tl, _), b in bins.items() if tl == 513} == {2} and any(b != 2 for (tl, _), b in bins.items() if tl == 512)
    assert {b for (_, w), b in bins.items() if w in (31, 32, 47, 48, 63, 64) and b != 2} >= {0, 3, 1}
    assert any(b == 2 for (tl, w), b in bins.items() if w == 64 and tl <= 512)
    run, ws = _glb_bins(mode, p, pool, tasks)
    short = tasks["tlen"] <= 512
    assert (run[~short] == 2).all()
    if mode == "own":  # each side of each band switch on the kernel the dispatcher names for it, four tasks a side
        for w, b in ((31, 0), (32, 3), (47, 3), (48, 1), (63, 1), (64, 2)):
            on = run[short & (tasks["w"] == w)]
            assert len(on) >= 4 and (on == b).all(), (w, on)
    elif mode != "wave":  # the band pass narrows these lightly mutated pairs, so the device must bin them by the narrowed band
        assert (ws[short] <= tasks["w"][short]).all() and (ws[short] < tasks["w"][short]).any()
        assert (run[short] == [br.lane_bin(int(w)) for w in ws[short]]).all()
    _cmp_glb_bins(ctx, mode, p, pool, tasks, words, f"{mode} shapes")

    for oo, lane_side in ((3999, True), (4000, False)):  # a parameter-level switch: two batches on the same context
        p = kswlib.make_params(o_del=oo - 1999, e_del=1, o_ins=1999, e_ins=1)
        pool, tasks, words = dg.gen_glb_shape_edges(rng, per=2)
        t0 = tasks[0]
        assert (dg.glb_lane_bin(p, int(t0["qlen"]), 20, 20, 512) != 2) == lane_side
        run = _glb_bins(mode, p, pool, tasks)[0]
        assert (run != 2).any() == (lane_side and mode != "wave")
        _cmp_glb_bins(ctx, mode, p, pool, tasks, words, f"{mode} o_del+o_ins={oo}")

    # deep scores in the wave kernel: the LDS / HBM-scratch variant is chosen once per batch (global_kernel.hip:288), so each
    # length gets a batch of its own
    low = {True: 0, False: 0}
    for p in (kswlib.make_params(a=127, b=127, o_del=1000, e_del=127, o_ins=900, e_ins=100),
              kswlib.make_params(a=64, mat=dg.big_matrix(rng, 64), o_del=300, e_del=30, o_ins=200, e_ins=40),
              kswlib.make_params(o_del=70000, e_del=1, o_ins=6, e_ins=1), kswlib.make_params(o_del=0, e_del=65537, o_ins=0, e_ins=65537)):
        for L, lds in ((200, True), (1200, False)):
            pool, tasks, words = dg.gen_glb_deep(rng, lens=(L,), per=3)
            assert dg.glb_wave_lds(tasks) == lds
            assert all(dg.glb_lane_bin(p, int(t["qlen"]), int(t["tlen"]), int(t["w"]), min(int(tasks["tlen"].max()), 512)) == 2 for t in tasks)
            res = _cmp_glb_bins(ctx, mode, p, pool, tasks, words, f"{mode} deep {L}")
            low[lds] = min(low[lds], int(res["score"].min()))
    assert low[True] < -100_000 and low[False] < -1_000_000
    ctx.close()


# ---- global: real scores across the lane kernels' 16-bit domain ---------------------------------------------------------

# The contexts every family runs on, and what glbbin_ref.expected_bins must be told about each
LANE_CTX = {
    "own-exact": ({"BMH_GLB_EXACT": "7", "BMH_GLB_NARROW": "0"}, dict(narrow=False, exact=7)),
    "narrowed": ({"BMH_GLB_EXACT": "7"}, dict(narrow=True, exact=7)),
    "own-c32": ({"BMH_GLB_EXACT": "0", "BMH_GLB_NARROW": "0"}, dict(narrow=False, exact=0)),
    "own-c64": ({"BMH_GLB_EXACT": "0", "BMH_GLB_NARROW": "0", "BMH_GLB_C32": "0"}, dict(narrow=False, exact=0, c32=0)),
    "own-masked": ({"BMH_GLB_NARROW": "0", "BMH_GL_FAST": "0"}, dict(narrow=False, exact=7)),  # (BMH_GLB_EXACT at its default)
}
LANE_FAMILIES = {
    "deep-negative-equal": lambda: dg.gen_glb_deep_negative_equal(np.random.default_rng(7310)),
    "threshold": dg.gen_glb_threshold,
    "deep-negative-unequal": lambda: dg.gen_glb_deep_negative_unequal(np.random.default_rng(7311)),
    "empty-target": lambda: dg.gen_glb_empty_target(np.random.default_rng(7312)),
    "deep-positive": lambda: dg.gen_glb_deep_positive(np.random.default_rng(7313)),
    "extreme-gaps": dg.gen_glb_extreme_gaps,
    "n-bases": lambda: dg.gen_glb_n_bases(np.random.default_rng(7314)),
}


@pytest.fixture(scope="module")
def lane_family():
    """name -> [(label, params, (pool, tasks, words), (oracle results, oracle CIGAR pool))], generated and run through the oracle once;
    (name, "bands") -> {label: glbband_ref.expected_bands of that batch}, worked out once as well."""
    cache = {}

    def get(name, what="batches"):
        if name not in cache:
            cache[name] = [(label, p, batch, kswlib.orc_global_batch_mt(p, *batch, nthreads=8)[:2]) for label, p, batch in LANE_FAMILIES[name]()]
        if what == "bands" and (name, what) not in cache:
            cache[name, what] = {label: gr.expected_bands(p, pool, tasks) for label, p, (pool, tasks, _), _ in cache[name]}
        return cache[name, what] if what == "bands" else cache[name]
    return get


@pytest.mark.parametrize("mode", list(LANE_CTX))
@pytest.mark.parametrize("family", list(LANE_FAMILIES))
def test_global_lane_kernels_across_their_domain(lane_family, family, mode):
    """Real scores from -11129 to +11684 (test_score_domain_cpu.py pins the depth each family reaches in each bin to the reference),
    gap opens up to 3999 in sum, gap extensions up to 2596, matrix entries of +-127 and N bases, on global_narrow_kernel and on
    global_lane_kernel<32|64|96|128>: every result field and CIGAR word is the oracle's, the device's per-bin task counts are the
    dispatcher's as glbbin_ref.py restates it, and with the band pass on its per-task bands are glbband_ref.py's."""
    env, rule = LANE_CTX[mode]
    ctx = _ctx_with(env)
    try:
        for label, p, (pool, tasks, words), (want, wcig) in lane_family(family):
            what = f"{family} / {label} / {mode}: "
            ctx.set_params(p)
            res, cig = ctx.global_batch(pool, tasks, words)
            bands = lane_family(family, "bands")[label] if rule["narrow"] else None
            counts, expect = ctx.last_global_bin_counts(), br.expected_counts(p, pool, tasks, bands=bands, **rule)
            print(f"{what}bins {counts.tolist()} scores {int(want['score'].min())} .. {int(want['score'].max())}")
            bad = np.nonzero(res != want)[0]
            if len(bad):  # which scores go wrong, before the assertion names the first task
                print(f"{what}{len(bad)} differ; oracle scores of those {sorted(set(want['score'][bad].tolist()))[:4]} .. {int(want['score'][bad].max())}, "
                      f"device scores {sorted(set(res['score'][bad].tolist()))[:4]}")
            dc.assert_glb(res, cig, want, wcig, tasks, what)
            assert (counts == expect).all() and expect[2] == 0 and expect[4] == 0, f"{what}bin counts {counts.tolist()}, the rule gives {expect.tolist()}"
            if rule["narrow"]:
                assert np.array_equal(ctx.last_global_bands(len(tasks)), bands), what
    finally:
        ctx.close()


def test_global_deep_scores_through_the_device_entry(lane_family):
    """bmh_global_batch_device on the deep-negative family: tasks, pool and results stay on the device, the slab is sized from the
    context's capacity hint (as test_global_exact_gpu.py's sparse-order case works it out)."""
    ctx = _ctx_with({"BMH_GLB_EXACT": "7"})
    try:
        for label, p, (pool, tasks, words), (want, wcig) in lane_family("deep-negative-equal"):
            ctx.set_params(p)
            ctx.set_qcap(int(tasks["qlen"].max()))
            g = dc.Glb(pool, tasks, words)
            g.run(ctx)
            ctx.sync()
            counts = ctx.last_global_bin_counts()
            res, cig = g.result()
            dc.assert_glb(res, cig, want, wcig, tasks, f"device entry / {label}: ")
            rows_cap = min(int(tasks["qlen"].max()) + 2 * int(p["w"]) + 64, gr.ROWS_CAP)
            expect = br.expected_counts(p, pool, tasks, rows_cap=rows_cap)
            assert (counts == expect).all() and expect[2] == 0, (label, counts.tolist(), expect.tolist())
    finally:
        ctx.close()


# ---- local Smith-Waterman -----------------------------------------------------------------------------------------------

SW_SETS = [kswlib.make_params(a=1, b=4), kswlib.make_params(a=2, b=4), kswlib.make_params(a=3, b=5, o_del=20, e_del=5, o_ins=30, e_ins=3),
           kswlib.make_params(a=127, b=127, o_del=200, e_del=55, o_ins=150, e_ins=100)]


@pytest.mark.parametrize("mode", list(SW_ENV))
def test_sw_on_both_sides_of_every_switch(mode):
    """sw_dispatch.hip:32-42, sw_common.h:45-50 and sw_wave.hip:190-193: byte mode qlen*max + shift of 254 / 255, word mode
    510 / 512 (a=2: qlen 253 / 254), padded queries of 80/81, 160/161 and 256/257 columns, scaled matrices, qlen*max(mat) =
    31999.  The cases of each parameter set go in two batches: queries of up to 320 columns, which the default path hands to
    sw_wave_kernel as a whole, and the longer ones, which take the register / slab routing.  `seen` records the kernel each
    task takes in this mode (domaingen.sw_kernel_of)."""
    ctx = _ctx_with(SW_ENV[mode])
    rng = np.random.default_rng(7400)
    seen = set()
    for k, p in enumerate(SW_SETS + [kswlib.make_params(a=100, mat=dg.big_matrix(rng, 100), o_del=254, e_del=1, o_ins=1, e_ins=254)]):
        cases = dg.sw_edge_cases(p)
        mx, sh = dg.max_mat(p), dg.sw_shift(p)
        for part in ([c for c in cases if c[0] <= 320], [c for c in cases if c[0] > 320]):
            if not part:
                continue
            pool, tasks = dg.gen_sw_edges(rng, p, part, per=3)
            assert dg.sw_wave_fits(tasks) == (part[0][0] <= 320)
            for t, kern in zip(tasks, dg.sw_kernel_of(p, tasks, mode)):
                q, x = int(t["qlen"]), int(t["xtra"])
                seen.add(("byte" if x & kswlib.KSW_XBYTE else "word", q * mx + sh, kern))
            _cmp_sw(ctx, p, pool, tasks, f"{mode} set {k}, queries {'<=' if part[0][0] <= 320 else '>'} 320")
    byte = {(v, kern) for m, v, kern in seen if m == "byte"}
    word = {(v, kern) for m, v, kern in seen if m == "word"}
    top = {"wave": ("wave", "wave"), "lane": (6, 7), "generic": ("generic", "generic")}[mode]
    assert (254, top[0]) in byte and (255, "generic") in byte        # the byte overflow edge, sw_dispatch.hip:39 / sw_common.h:49
    assert (510, top[1]) in word and (512, "generic") in word        # the word edge, sw_dispatch.hip:37 / sw_common.h:49
    if mode == "lane":
        assert {0, 1, 6} <= {kern for _, kern in byte} and 7 in {kern for _, kern in word}
    p = kswlib.make_params(a=11, b=20, o_del=40, e_del=10, o_ins=40, e_ins=10)
    pool, tasks = dg.gen_sw_edges(rng, p, [(2909, dg.X_START), (2909, 0)], per=1)
    assert (tasks["qlen"].astype(int) * 11 == 31999).all()
    _cmp_sw(ctx, p, pool, tasks, f"{mode} qlen*max = 31999")
    ctx.close()


@pytest.mark.parametrize("mode", list(SW_ENV))
def test_sw_gap_costs_up_to_255(mode):
    """Byte and word mode under gap costs up to 255.  Where o+e reaches 256, ksw_u8 wraps it in its 8-bit lanes and the kernels
    refuse byte-mode tasks (BMH_E_RANGE); word-mode tasks stay exact, and so does the next batch on the same context."""
    pkg = load_package()
    ctx = _ctx_with(SW_ENV[mode])
    rng = np.random.default_rng(7500)
    for (o_del, e_del, o_ins, e_ins), wrap in dg.sw_gap_param_sets():
        p = kswlib.make_params(a=1, b=4, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins)
        assert dg.wraps(p) == wrap
        pool, tasks = kswgen.gen_sw_fuzz(rng, 500, p)
        want, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=8)
        tasks = tasks[want["rsv"] == 0]
        byte = (tasks["xtra"] & kswlib.KSW_XBYTE) != 0
        assert byte.sum() > 150 and (~byte).sum() > 100
        if wrap:
            ctx.set_params(p)
            with pytest.raises(pkg.BmhError) as e:
                ctx.sw_batch(pool, tasks)
            assert e.value.code == pkg.BMH_E_RANGE and "byte mode needs o_del+e_del and o_ins+e_ins below 256" in str(e.value)
            tasks = tasks[~byte]
        _cmp_sw(ctx, p, pool, tasks, f"{mode} gaps {(o_del, e_del, o_ins, e_ins)}")
    ctx.close()


def test_sw_large_batch_reaches_the_lane_kernels():
    """More than 32 768 tasks: the register kernels serve the batch without any switch (sw_dispatch.hip:102), here with tasks on
    both sides of the byte, word and padding edges."""
    ctx = _ctx_with({})
    rng = np.random.default_rng(7600)
    p = kswlib.make_params(a=1, b=4, o_del=200, e_del=55, o_ins=250, e_ins=5)
    cases = [(q, x) for q, x in dg.sw_edge_cases(p) if q <= 260]
    pb = kswgen.PoolBuilder(kswlib.SW_TASK)
    for k in range(33000):
        q, x = cases[k % len(cases)]
        dg.sw_task(pb, rng, q, q + int(rng.integers(10, 120)), x | 19)
    pool, tasks = pb.finish()
    assert len(tasks) > 32768
    bins = {dg.sw_bin(p, int(t["qlen"]), int(t["xtra"])) for t in tasks}
    assert {0, 1, 2, 6, 7} <= bins
    _cmp_sw(ctx, p, pool, tasks, "large batch")
    ctx.close()


# ---- refusals exactly at the limit --------------------------------------------------------------------------------------

def test_refusals_exactly_at_the_limit_leave_the_context_exact():
    pkg = load_package()
    ctx = _ctx_with({})
    rng = np.random.default_rng(7700)

    def refused(call, why):  # BMH_E_RANGE, and from the check named by `why` (the context's last error)
        with pytest.raises(pkg.BmhError) as e:
            call()
        assert e.value.code == pkg.BMH_E_RANGE and why in str(e.value), str(e.value)

    # seed record: o+e of 65536 and e of 16384 (ext_gaps_too_large, bmh_ctx.h)
    spool, seeds = _seeds_at(rng, 150, 8)
    for p in (kswlib.make_params(o_del=65535, e_del=1), kswlib.make_params(o_ins=6, e_ins=16384)):
        ctx.set_params(p)
        refused(lambda: ctx.seedext_batch(spool, seeds), EXT_GAPS_MSG)

    # extension: h0 + qlen*max(mat) = 32001 (api.hip:484), then 32000 on the same context
    p = kswlib.make_params(a=100, b=127, o_del=600, e_del=100, o_ins=600, e_ins=100)
    ctx.set_params(p)
    pool, tasks = dg.gen_ext_edges(rng, p, qlens=(64, 250), per=4)
    over = tasks.copy()
    over["h0"][0] = dg.LIMIT + 1 - int(over["qlen"][0]) * 100
    refused(lambda: ctx.extend_batch(pool, over), "h0 + qlen*max(mat) exceeds the 16-bit score range")
    _cmp_ext(ctx, p, pool, tasks, "extension after a refusal")

    # fused seed record: l_query*max(max_mat, a) = 32001 (api.hip:641)
    p3 = kswlib.make_params(a=3, b=4)
    ctx.set_params(p3)
    spool, seeds = _seeds_at(rng, 10667, 2)
    refused(lambda: ctx.seedext_batch(spool, seeds), "l_query*max(max(mat), a) exceeds the 16-bit score range")
    p = kswlib.make_params(a=100, b=127, o_del=600, e_del=100, o_ins=600, e_ins=100)
    spool, seeds = _seeds_at(rng, 320, 64)
    _cmp_seed(ctx, p, spool, seeds, "seed record after a refusal")

    # Smith-Waterman: qlen*max(mat) = 32000 (api.hip:896) and a gap cost of 256 (sw_dispatch.hip:120)
    p = kswlib.make_params(a=125, b=127, o_del=100, e_del=50, o_ins=100, e_ins=50)
    ctx.set_params(p)
    pool, tasks = dg.gen_sw_edges(rng, p, [(256, dg.X_START)], per=1)
    refused(lambda: ctx.sw_batch(pool, tasks), "qlen*max(mat) below the 16-bit score range")
    pool, tasks = dg.gen_sw_edges(rng, p, [(255, dg.X_START), (40, 0), (2, kswlib.KSW_XBYTE | dg.X_SCORE)], per=3)
    _cmp_sw(ctx, p, pool, tasks, "SW after the qlen refusal")
    for gaps in ((256, 1, 6, 1), (6, 256, 6, 1), (6, 1, 256, 1), (6, 1, 6, 256)):
        bad = kswlib.make_params(o_del=gaps[0], e_del=gaps[1], o_ins=gaps[2], e_ins=gaps[3])
        ctx.set_params(bad)
        pool, tasks = kswgen.gen_sw_materescue(rng, 50, bad, read_len=(300, 300))  # word mode: only the gap limit applies
        assert (tasks["xtra"] & kswlib.KSW_XBYTE == 0).all()
        refused(lambda: ctx.sw_batch(pool, tasks), "gap penalties below 256")
        p = kswlib.make_params(o_del=min(gaps[0], 255), e_del=min(gaps[1], 255) if gaps[1] > 1 else 1,
                               o_ins=min(gaps[2], 255), e_ins=min(gaps[3], 255) if gaps[3] > 1 else 1)
        pool, tasks = kswgen.gen_sw_materescue(rng, 200, p)
        if dg.wraps(p):  # refused in byte mode (test_sw_gap_costs_up_to_255): word mode here
            tasks["xtra"] &= ~np.uint32(kswlib.KSW_XBYTE)
        _cmp_sw(ctx, p, pool, tasks, f"SW after the gap refusal {gaps}")
    ctx.close()


def test_sw_device_entry_refuses_wrapping_byte_mode():
    """bmh_sw_batch_device finds byte-mode tasks on the device (sw_caps_kernel) and refuses them where o+e wraps in ksw_u8's
    8-bit lanes; the next device-resident batch on the same context is exact."""
    import torch
    pkg = load_package()
    ctx = _ctx_with({})
    rng = np.random.default_rng(7800)
    dev = torch.device("cuda:0")

    def run(p, pool, tasks):
        ctx.set_params(p)
        d_pool = torch.from_numpy(pool).to(dev)
        d_tasks = torch.from_numpy(tasks.view(np.uint8)).to(dev)
        d_res = torch.zeros(len(tasks) * kswlib.SW_RES.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.sw_batch_device(d_pool.data_ptr(), d_tasks.data_ptr(), len(tasks), d_res.data_ptr())
        ctx.sync()
        return d_res.cpu().numpy().view(kswlib.SW_RES)

    p = kswlib.make_params(o_del=128, e_del=128, o_ins=1, e_ins=1)
    pool, tasks = kswgen.gen_sw_materescue(rng, 300, p)  # 150 bp, a = 1: byte mode
    assert (tasks["xtra"] & kswlib.KSW_XBYTE != 0).all()
    with pytest.raises(pkg.BmhError) as e:
        run(p, pool, tasks)
    assert e.value.code == pkg.BMH_E_RANGE and "byte mode needs o_del+e_del and o_ins+e_ins below 256" in str(e.value)
    tasks["xtra"] &= ~np.uint32(kswlib.KSW_XBYTE)  # the same tasks in word mode are served, exactly
    want, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=8)
    got = run(p, pool, tasks)
    for f in kswlib.SW_FIELDS:
        assert (got[f] == want[f]).all(), f
    p = kswlib.make_params()
    pool, tasks = kswgen.gen_sw_materescue(rng, 300, p)
    want, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=8)
    got = run(p, pool, tasks)
    for f in kswlib.SW_FIELDS:
        assert (got[f] == want[f]).all(), f
    ctx.close()
