"""Every DP kernel on sequence pools and CIGAR pools past 4 GiB, and on BMH_F_TPAC targets at coordinates past 2^32.

tests/bigpool.py relocates a batch whose expected results the oracle computed on a small pool to a base inside a device pool of up
to a little over 8 GiB (placements: across byte 2^32, above 2^32 + 2^31, across byte 2^33), with tasks that view one string lying
across the boundary and a decoy where a truncated offset would land.  Every kernel family behind the four *_device entry points
must return the oracle's records bit for bit.  Then: a CIGAR pool of 2^32 words (lane and wave kernels), once the host-buffer
entry points and their transfer path with a host pool just past 4 GiB, and extension, fused per-seed and Smith-Waterman tasks
whose targets are coordinates in the top 5 Mbp of either strand of a 2.3 Gbp resident reference.

One device pool per placement, allocated once and refilled per batch; tests/test_pool_offsets_cpu.py shows on the CPU that the
oracle itself is 64-bit clean on these pools and that the inputs discriminate."""
import numpy as np
import pytest

import bigpool as bp
import devcalls as dc
import globallong as gl
import kswgen
import kswlib
import pacwin
import widegen as wg
import widesw
from __graft_entry__ import load_package
from test_device_entry_gpu import _tg, concat_seeds, long_seeds
from test_kernel_families_gpu import _ctx_with
from test_sw_gpu import _sw_ctx

pytestmark = pytest.mark.gpu

GIB = 1 << 30
P = kswlib.make_params()
LANEX_MIN_TASKS = 4096   # kLanexMinTasks, extend_dispatch.hip
GRP_TCAP = 1024          # kGrpTcapHost, bmh_ctx.h
QCAP = 600               # bmh_ctx_set_qcap for the *_device calls: the longest query of the ordinary batches


def _need(nbytes):
    """No case is left out on a device of 64 GiB or more; a smaller one skips and says what the case allocates."""
    import torch
    total = torch.cuda.mem_get_info()[1]
    if total < 64 * GIB:
        pytest.skip(f"allocates {nbytes / GIB:.1f} GiB at once and runs on devices of 64 GiB or more; this one has {total / GIB:.1f} GiB")


# ---- the batches and what the oracle says about them (small pools: once per module) ---------------------------------------

class Case:
    def __init__(self, batch, p=P):
        self.b, self.p = batch, p
        t = batch.tasks
        if batch.kind == "ext":
            self.want = kswlib.orc_extend_batch(p, batch.pool, t, nthreads=8)[0]
        elif batch.kind == "seed":
            self.want = kswlib.orc_seedext_batch(p, batch.pool, t, nthreads=8)[0]
        elif batch.kind == "sw":
            self.want = kswlib.orc_sw_batch(p, batch.pool, t, nthreads=8)[0]
            assert (self.want["rsv"] == 0).all()
        else:
            self.want, self.wcig, _ = kswlib.orc_global_batch_mt(p, batch.pool, t, batch.words, nthreads=8)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20261)
    c = {}
    c["ext"] = Case(bp.ext_batch(rng, n_side=1200, long_targets=32))
    many = bp.ext_batch(rng, n_side=300, n_views=72, read_len=(300, 400), qlens=(130, 160, 200, 230, 256))
    many.tasks, many.fam = np.concatenate([many.tasks] * 20), np.concatenate([many.fam] * 20)   # twenty records per sequence pair
    c["ext_many"] = Case(many)
    wide = bp.ext_batch(rng, n_side=500, n_views=72)
    to_wide = (wide.fam != bp.ORD) | (np.arange(len(wide.tasks)) % 4 != 0)   # every view of both families, 3 ordinary tasks in 4
    wide.tasks["h0"][to_wide] = 31990           # h0 + qlen * max(mat) > 32000: per-task routing to the int32 kernel
    c["ext_wide"] = Case(wide)
    c["seed"] = Case(bp.seed_batch(rng))
    c["seed_w8"] = Case(c["seed"].b, kswlib.make_params(w=8))
    tg = _tg()                                  # the package's own seed generator and long reads as the ordinary halves
    sides = [concat_seeds(tg.generate_seeds(P, 400, "mixed100-300", seed=77 + k), long_seeds(rng, [450, 500, 560, 590] * 4)) for k in (0, 1)]
    c["seed_tg"] = Case(bp.seed_batch(rng, sides=sides))
    # 70 views per family and 220 regions per side in each of the five band classes: every lane bin gets the caps of its own
    c["glb"] = Case(bp.glb_batch(rng, n_side=300, n_views=350, view_len=(9, 500), n_class=1100))
    c["glb_short"] = Case(bp.glb_batch(rng, n_side=260, view_len=(9, 56), realistic=False))
    lng = gl.gen_long(rng, [(10500, 40, "cigar")])
    c["glb_ring"] = Case(bp.glb_batch(rng, n_side=200, n_views=64, extra=(lng[0], lng[1])))
    c["sw"] = Case(bp.sw_batch(rng, P))
    c["sw_long"] = Case(bp.sw_batch(rng, P, n_side=200, n_views=64, qlen=(330, 600), flank=(20, 300)))
    return c


# ---- one device pool per placement -----------------------------------------------------------------------------------------

class DevPool:
    """A zeroed device buffer with bigpool.PAD bytes in front of offset 0; load() copies one batch's block and decoys in and takes
    the previous batch's out again."""

    def __init__(self, placement, nbytes):
        import torch
        _need(nbytes)
        self.placement, self.nbytes = placement, nbytes
        self.t = torch.zeros(bp.PAD + nbytes, dtype=torch.uint8, device=dc.dev())
        self.loaded, self.runs = None, []

    def data_ptr(self):
        return self.t.data_ptr() + bp.PAD

    def load(self, batch):
        import torch
        if self.loaded is batch:
            return self
        for off, n in self.runs:
            self.t[bp.PAD + off:bp.PAD + off + n] = 0
        self.runs = []
        assert batch.total(self.placement) <= self.nbytes
        for off, run in batch.segments(self.placement):
            self.t[bp.PAD + off:bp.PAD + off + len(run)] = torch.from_numpy(np.ascontiguousarray(run)).to(dc.dev())
            self.runs.append((off, len(run)))
        torch.cuda.synchronize()
        self.loaded = batch
        return self


@pytest.fixture(scope="module", params=bp.PLACEMENTS)
def place(request, cases):
    import torch
    pl = request.param
    pool = DevPool(pl, max(c.b.total(pl) for c in cases.values()) + 4096)
    yield pool
    pool.t = None
    del pool
    torch.cuda.empty_cache()


def _census(case, pool, what):
    """The caps of a straddling placement, asserted per (entry point, kernel family, placement)."""
    c = case.b.census(pool.placement)
    if bp.BOUNDARY[pool.placement] is not None:
        bp.assert_caps(c, case.b.kind in ("ext", "sw"), what)
    else:
        assert c["ord"]["above"] >= 2 * bp.MIN_SIDE and c["T"]["above"] >= bp.MIN_VIEWS and c["Q"]["above"] >= bp.MIN_VIEWS
    return c


def _census_of(case, pool, sel, what):
    """The same caps for the part of the batch that routing sends to one kernel."""
    b = bp.BOUNDARY[pool.placement]
    if b is not None:
        c = bp.census(case.b.moved(pool.placement)[sel], case.b.fam[sel], b)
        bp.assert_caps(c, case.b.kind in ("ext", "sw"), what, edges=False)


def _run(ctx, case, pool, order=None):
    """One *_device call of the case's batch against the loaded pool -> what devcalls' result() gives."""
    pool.load(case.b)
    moved = case.b.moved(pool.placement)
    stub = np.zeros(16, np.uint8)
    if case.b.kind == "ext":
        call = dc.Ext(stub, moved, order)
    elif case.b.kind == "seed":
        call = dc.Seed(stub, moved)
    elif case.b.kind == "sw":
        call = dc.Sw(stub, moved)
    else:
        call = dc.Glb(stub, moved, case.b.words, order)
    call.pool = pool
    call.run(ctx)
    ctx.sync()
    return call.result()


def _check(ctx, case, pool, what, order=None):
    got = _run(ctx, case, pool, order)
    t = case.b.moved(pool.placement)
    what = f"{what} at {pool.placement}: "
    if case.b.kind == "ext":
        dc.assert_ext(got, case.want, t, what)
    elif case.b.kind == "seed":
        dc.assert_seed(got, case.want, t, what)
    elif case.b.kind == "sw":
        dc.assert_sw(got, case.want, t, what)
    else:
        dc.assert_glb(got[0], got[1], case.want, case.wcig, t, what)
        assert (got[0]["n_cigar"][t["cigar_cap"] > 0] > 0).all()


# ---- bmh_extend_batch_device ----------------------------------------------------------------------------------------------

def _ext_bins(tasks):
    q = tasks["qlen"]
    return [int((q <= 32).sum()), int(((q > 32) & (q <= 64)).sum()), int(((q > 64) & (q <= 128)).sum()),
            int(((q > 128) & (q <= 256)).sum()), int(((q > 256) & (q <= 512)).sum()), int((q > 512).sum())]


@pytest.mark.parametrize("mode", ["lane", "lanex4", "reg", "grp", "lds"])
def test_extend_families(place, cases, mode):
    case = cases["ext"]
    _census(case, place, f"extend {mode}: ")
    t = case.b.tasks
    bins = _ext_bins(t)
    assert min(bins) > 0 and ((t["qlen"] > 64) & (t["qlen"] <= 96)).sum() > 0 and ((t["qlen"] > 96) & (t["qlen"] <= 128)).sum() > 0
    if mode == "grp":
        assert ((t["tlen"] > GRP_TCAP) & (t["qlen"] <= 256)).sum() >= 16
    ctx = _ctx_with({"BMH_EXT_MODE": mode})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    ctx.set_kernel_timing(True)
    _check(ctx, case, place, f"extend {mode}")
    ms = ctx.last_extend_bin_ms()
    claimed = {"lane": (0, 1, 2, 3, 5), "lanex4": (0, 1, 2, 3, 4, 5), "reg": (0, 1, 2, 3, 5), "grp": (0, 1, 2, 3, 5), "lds": (5,)}[mode]
    assert all(ms[b] >= 0 for b in claimed), f"{mode}: per-bin times {ms}"
    ctx.set_kernel_timing(False)
    order = np.random.default_rng(5).permutation(len(t)).astype(np.uint32)
    _check(ctx, case, place, f"extend {mode} with d_order", order)
    ctx.close()


def test_extend_many_long_flanks_take_two_lanes_per_task(place, cases):
    case = cases["ext_many"]
    _census(case, place, "extend lanex<2>: ")
    assert _ext_bins(case.b.tasks)[3] > LANEX_MIN_TASKS
    ctx = _ctx_with({"BMH_EXT_MODE": "lane"})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    _check(ctx, case, place, "extend lanex<2>")
    _check(ctx, case, place, "extend lanex<2>, second launch (hinted bins)")
    ctx.close()


@pytest.mark.parametrize("forced", [True, False], ids=["BMH_EXT_MODE=wide", "per-task routing"])
def test_extend_wide(place, cases, forced):
    case = cases["ext" if forced else "ext_wide"]
    _census(case, place, "extend wide: ")
    ctx = _ctx_with({"BMH_EXT_MODE": "wide"} if forced else {})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    ctx.set_wide_extension(True)
    n_wide = len(case.b.tasks) if forced else wg.wide_count(P, case.b.tasks)
    assert n_wide >= 200
    if not forced:
        _census_of(case, place, np.array([wg.goes_wide(P, int(x["qlen"]), int(x["h0"])) for x in case.b.tasks]), "extend wide, routed: ")
    _check(ctx, case, place, "extend wide")
    assert ctx.extend_wide_stats()[0] == n_wide
    order = np.random.default_rng(6).permutation(len(case.b.tasks)).astype(np.uint32)
    _check(ctx, case, place, "extend wide with d_order", order)
    ctx.close()


# ---- bmh_seedext_batch_device ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", ["default", 8])
@pytest.mark.parametrize("mode", ["default", "reg"])
def test_seedext_families(place, cases, mode, w):
    case = cases["seed" if w == "default" else "seed_w8"]
    _census(case, place, f"seedext {mode} w={w}: ")
    ctx = _ctx_with({} if mode == "default" else {"BMH_EXT_MODE": mode})
    ctx.set_params(case.p)
    ctx.set_qcap(QCAP)
    _check(ctx, case, place, f"seedext {mode} w={w}")
    if w == 8:   # both retry lists re-read the derived offsets: seeds that ran at 2w, some of them on both sides (four extensions)
        views = case.b.fam != bp.ORD
        assert (case.want["w"][views] == 16).sum() >= 16 and (case.want["n_ext"] == 4).sum() >= 1
    _check(ctx, case, place, f"seedext {mode} w={w}, second call (hinted bins)")
    ctx.close()


def test_seedext_generator_and_long_read_seeds(place, cases):
    """The package's seed generator (mixed 100-300 bp) and long-read seeds (flanks up to 560) as the halves below and above."""
    case = cases["seed_tg"]
    _census(case, place, "seedext taskgen: ")
    ctx = _ctx_with({})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    _check(ctx, case, place, "seedext taskgen + long seeds")
    ctx.close()


# ---- bmh_global_batch_device ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", ["1", "0"])
def test_global_lane_kernels(place, cases, fast):
    case = cases["glb"]
    _census(case, place, f"global lane BMH_GL_FAST={fast}: ")
    route = gl.route(P, case.b.tasks)
    for b in (0, 3, 1, 2):   # w <= 31, 32-47, 48-63, and the wave kernel's wider bands: each kernel's share meets the caps
        _census_of(case, place, route == b, f"global lane bin {b}: ")
    ctx = _ctx_with({"BMH_GLB_MODE": "lane", "BMH_GL_FAST": fast})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    ctx.set_kernel_timing(True)
    _check(ctx, case, place, f"global lane BMH_GL_FAST={fast}")
    assert all(ms >= 0 for ms in ctx.last_global_bin_ms()), ctx.last_global_bin_ms()
    order = np.random.default_rng(7).permutation(len(case.b.tasks)).astype(np.uint32)
    _check(ctx, case, place, "global lane with d_order", order)
    ctx.close()


@pytest.mark.parametrize("variant", ["slab", "lds"])
def test_global_wave_kernel(place, cases, variant):
    """BMH_GLB_MODE=wave: every task on global_kernel; the *_device call sizes the direction bytes from the capacity hint -- qcap
    64 keeps them in LDS (64 columns x 328 rows), qcap 600 puts them in the HBM slab."""
    case = cases["glb" if variant == "slab" else "glb_short"]
    _census(case, place, f"global wave {variant}: ")
    qcap = QCAP if variant == "slab" else 64
    assert int(case.b.tasks["qlen"].max()) <= qcap
    w4 = max(int(P["w"]) * 4, 100)
    assert (16 * qcap + 48 + min(qcap, 2 * w4 + 1) * (qcap + 2 * int(P["w"]) + 64) <= 64 * 1024) == (variant == "lds")
    ctx = _ctx_with({"BMH_GLB_MODE": "wave"})
    ctx.set_params(P)
    ctx.set_qcap(qcap)
    ctx.set_kernel_timing(True)
    _check(ctx, case, place, f"global wave {variant}")
    assert ctx.last_kernel_ms() >= 0
    ctx.close()


def test_global_band_ring(place, cases):
    case = cases["glb_ring"]
    _census(case, place, "global ring: ")
    assert gl.long_count(P, case.b.tasks) == 1 and int(case.b.tasks["qlen"].max()) > gl.GLB_LDS_QCAP
    ctx = _ctx_with({})
    ctx.set_params(P)
    ctx.set_qcap(12000)
    _check(ctx, case, place, "global ring")
    assert ctx.global_long_stats()[0] == 1
    ctx.close()


# ---- bmh_sw_batch_device --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["wave", "lane", "generic"])
def test_sw_families(place, cases, mode):
    case = cases["sw"]
    _census(case, place, f"sw {mode}: ")
    t = case.b.tasks
    views = case.b.fam != bp.ORD
    both = kswlib.BMH_F_QREV | kswlib.BMH_F_QCOMP
    assert ((t["flags"][views] & both) == both).sum() >= 8          # reversed and complemented mates among the views
    n_with_N = sum(1 for k in np.nonzero(views)[0] if (kswlib.sw_task_seqs(case.b.pool, t[k])[0] > 3).any())
    assert n_with_N >= 16                                           # ... and queries with an N (the scan of sw_dispatch.hip)
    ctx = _sw_ctx(mode)
    ctx.set_params(P)
    _check(ctx, case, place, f"sw {mode}")
    ctx.close()


def test_sw_long_kernel(place, cases):
    case = cases["sw_long"]
    _census(case, place, "sw long: ")
    n_long = widesw.long_count(P, case.b.tasks)
    assert n_long == len(case.b.tasks)                                # (the whole batch: _census's caps are the kernel's)
    ctx = _sw_ctx("wave")
    ctx.set_params(P)
    ctx.set_wide_sw(True)
    _check(ctx, case, place, "sw long")
    assert ctx.sw_wide_stats()[0] == n_long
    ctx.close()


# ---- a CIGAR pool past 2^30 words -----------------------------------------------------------------------------------------

GUARD = 64   # words checked on either side of every slot


@pytest.mark.parametrize("mode", ["lane", "wave"])
def test_cigar_pool_of_2_to_32_words(mode):
    """d_cigar of 2^32 words (16 GiB); slots just below and above word 2^30, 2^31 and ending at word 2^32.  From word 2^30 on the
    byte offset passes 2^32: at the byte offset cut to 32 bits stands a different, valid-looking CIGAR, so a wrapped write lands in
    bounds and is seen -- the expected words must be at cigar_off, and the filler and a guard band around every slot untouched."""
    import torch
    _need(16 * GIB)
    rng = np.random.default_rng(77 + len(mode))
    pool, tasks, _ = kswgen.gen_glb_realistic(rng, 240, read_len=(100, 300), hard=True)
    tasks = tasks[tasks["cigar_cap"] > 0][:192].copy()
    n, cap = len(tasks), int(tasks["cigar_cap"].max()) + 2 * GUARD
    assert n == 192
    # slot (i, j) of mark i starts (3 * j + i) * cap + GUARD words from it (with its guard bands: cap words), so that no two slots
    # are congruent mod 2^30 and no filler falls on a slot: below the mark for j < 0 -- for 2^32 the j = -1 slot ends on it
    marks = [1 << 30, 1 << 31, 1 << 32]
    per = n // 6
    offs = []
    for i, m in enumerate(marks):
        js = list(range(-per, per)) if i < 2 else list(range(-2 * per, 0))
        offs += [m + (3 * j + i) * cap + GUARD for j in js]
    offs = np.array(offs, dtype=np.int64)
    assert len(offs) == n and len(set((offs % (1 << 30)).tolist())) == n
    tasks["cigar_off"] = offs
    last = int(np.argmax(offs))
    tasks["cigar_cap"][last] = (1 << 32) - int(offs[last])   # cigar_off = 2^32 - cigar_cap
    assert int(tasks["cigar_cap"][last]) == cap - GUARD and (offs >= 1 << 30).sum() >= n // 2
    small = tasks.copy()
    small["cigar_off"] = np.arange(n) * cap
    want, wcig, _ = kswlib.orc_global_batch_mt(P, pool, small, n * cap, nthreads=8)
    d_cig = torch.zeros(1 << 32, dtype=torch.int32, device=dc.dev())
    FILL, LOW = 0x5A5A5A50, 0x00000F10                       # poison around the slots; the filler: a 241M operation
    wrapped = (offs * 4 % (1 << 32)) // 4
    for o, wr in zip(offs.tolist(), wrapped.tolist()):
        d_cig[o - GUARD:o + cap - GUARD] = FILL
    for o, wr in zip(offs.tolist(), wrapped.tolist()):
        if wr != o:
            d_cig[wr:wr + cap - 2 * GUARD] = LOW
    ctx = _ctx_with({"BMH_GLB_MODE": mode})
    ctx.set_params(P)
    ctx.set_qcap(QCAP)
    d_pool, d_tasks, d_res = dc.up(pool), dc.up(tasks), dc.poisoned(n * kswlib.GLB_RES.itemsize)
    torch.cuda.synchronize()
    ctx.global_batch_device(d_pool.data_ptr(), d_tasks.data_ptr(), n, d_res.data_ptr(), d_cig.data_ptr())
    ctx.sync()
    res = dc.down(d_res, kswlib.GLB_RES, n)
    bad = np.nonzero(res != want)[0]
    assert len(bad) == 0, f"{mode}: {len(bad)} results differ; first {tasks[bad[0]]}: gpu={res[bad[0]]} want={want[bad[0]]}"
    for k in range(n):
        o, wr, nc = int(offs[k]), int(wrapped[k]), int(res[k]["n_cigar"])
        slot = d_cig[o - GUARD:o + cap - GUARD].cpu().numpy().view(np.uint32)
        assert np.array_equal(slot[GUARD:GUARD + nc], wcig[k * cap:k * cap + nc]), f"{mode}: task {k} at word {o}: CIGAR words differ"
        kcap = int(tasks["cigar_cap"][k])                     # (a kernel may use its whole slot while it builds the CIGAR)
        assert nc <= kcap and (slot[:GUARD] == FILL).all() and (slot[GUARD + kcap:] == FILL).all(), f"{mode}: task {k} at word {o}: words outside the slot changed"
        if wr != o:
            low = d_cig[wr:wr + cap - 2 * GUARD].cpu().numpy().view(np.uint32)
            assert (low == LOW).all(), f"{mode}: task {k} at word {o} wrote at word {wr}: the byte offset was cut to 32 bits"
    assert (res["n_cigar"] > 0).all()
    ctx.close()
    del d_cig
    torch.cuda.empty_cache()


# ---- host-buffer entry points and the transfer path, once, at the smallest size that crosses -----------------------------

HOST_TOTAL = (1 << 32) + (64 << 20)


@pytest.fixture(scope="module")
def host_pools():
    """ONE host pool of 2^32 + 64 MiB holding the straddle32 layout of the extension, fused per-seed, global and Smith-Waterman
    batches' blocks in turn (a few megabytes each are rewritten; the 4 GiB are allocated once)."""
    _need(2 * HOST_TOTAL)
    big = np.zeros(bp.PAD + HOST_TOTAL, np.uint8)[bp.PAD:]
    state = {"runs": []}

    def load(batch):
        for off, n in state["runs"]:
            big[off:off + n] = 0
        state["runs"] = []
        for off, run in batch.segments("straddle32"):
            big[off:off + len(run)] = run
            state["runs"].append((off, len(run)))
        return big, batch.moved("straddle32")
    return load


def test_host_buffer_entry_points_past_4_gib(cases, host_pools):
    import torch
    pkg = load_package()
    ctx = _ctx_with({})
    ctx.set_params(P)
    # a resident pool: bmh_upload_pool, then the three calls that take pool = NULL
    ext = cases["ext"]
    big, moved = host_pools(ext.b)
    bp.assert_caps(ext.b.census("straddle32"), True, "host extend: ")
    ctx.upload_pool(big)
    dc.assert_ext(ctx.extend_batch(None, moved), ext.want, moved, "extend_batch(None) after upload_pool: ")
    # a task whose sequence ends one byte past pool_bytes is refused as at small sizes, and the context is exact afterwards
    over = moved[:4].copy()
    over["flags"][3], over["q_off"][3], over["qlen"][3] = 0, HOST_TOTAL - 9, 10
    with pytest.raises(pkg.BmhError) as e:
        ctx.extend_batch(None, over)
    assert e.value.code == pkg.BMH_E_ARG and "outside the sequence pool" in str(e.value)
    with pytest.raises(pkg.BmhError) as e:
        ctx.extend_batch(big, over)
    assert e.value.code == pkg.BMH_E_ARG and "outside the sequence pool" in str(e.value)
    over["qlen"][3] = 9                                      # ... and one that ends on the last byte is served
    assert ctx.extend_batch(None, over)[3] == kswlib.orc_extend_batch(P, big, over[3:4])[0][0]
    dc.assert_ext(ctx.extend_batch(None, moved), ext.want, moved, "extend_batch(None) after a refused batch: ")
    # the pool passed directly: the range checks on pool_bytes and the direct-copy branch of the transfer
    dc.assert_ext(ctx.extend_batch(big, moved), ext.want, moved, "bmh_extend_batch, pool passed: ")
    # two contexts on device 0, the split between the halves below and above the boundary
    q_lo, q_hi, _, t_lo, t_hi, _ = bp.spans(moved)
    lo = np.nonzero((ext.b.fam == bp.ORD) & (np.maximum(q_hi, t_hi) <= bp.TWO32))[0]
    hi = np.nonzero((ext.b.fam == bp.ORD) & (np.minimum(q_lo, t_lo) >= bp.TWO32))[0]
    k = min(len(lo), len(hi))
    assert k >= bp.MIN_SIDE
    sel = np.concatenate([lo[:k], hi[:k]])
    half, whalf = moved[sel], ext.want[sel]
    q_lo, q_hi, _, t_lo, t_hi, _ = bp.spans(half)
    assert (np.maximum(q_hi, t_hi)[:k] <= bp.TWO32).all() and (np.minimum(q_lo, t_lo)[k:] >= bp.TWO32).all()
    ctx2 = _ctx_with({})
    ctx2.set_params(P)
    dc.assert_ext(pkg.extend_batch_sharded([ctx, ctx2], big, half), whalf, half, "extend_batch_sharded: ")
    ctx2.close()
    for name in ("seed", "glb"):
        case = cases[name]
        big, moved = host_pools(case.b)
        ctx.upload_pool(big)
        if name == "seed":
            dc.assert_seed(ctx.seedext_batch(None, moved), case.want, moved, "seedext_batch(None): ")
        else:
            res, cig = ctx.global_batch(None, moved, case.b.words)
            dc.assert_glb(res, cig, case.want, case.wcig, moved, "global_batch(None): ")
    case = cases["sw"]
    big, moved = host_pools(case.b)
    dc.assert_sw(ctx.sw_batch(big, moved), case.want, moved, "bmh_sw_batch, pool passed: ")
    ctx.close()
    torch.cuda.empty_cache()


# ---- BMH_F_TPAC targets at coordinates past 2^32 ---------------------------------------------------------------------------

L_PAC = 2_300_000_011    # the 2.3 Gbp reference of tests/test_pac_resident_gpu.py: reverse-strand coordinates pass 2^32
TOP = 5_000_000          # positions are drawn from the top 5 Mbp of each strand


@pytest.fixture(scope="module")
def tpac():
    """Reads copied with errors from the top of either strand.  Per read: a left and a right extension, one fused per-seed record
    and one Smith-Waterman task, each addressed (a) by doubled coordinate with BMH_F_TPAC and (b) by the window's bytes in the pool."""
    rng = np.random.default_rng(4611)
    pac = rng.integers(0, 256, L_PAC // 4 + 1, dtype=np.uint8)
    F = kswlib
    pool, off = [], 0
    ext, seed, sw = ([], []), ([], []), ([], [])
    for k in range(900):
        L = int(rng.integers(60, 561))
        rev = k & 1
        lo, hi = (L_PAC, 2 * L_PAC) if rev else (0, L_PAC)
        margin = 100 + L
        pos = int(rng.integers(hi - TOP, hi - L - (0 if k % 9 == 0 else margin)))     # (every ninth window ends on the strand's end)
        read = pacwin.window(pac, L_PAC, pos, L).copy()
        mut = rng.random(L) < 0.03
        read[mut] = (read[mut] + rng.integers(1, 4, int(mut.sum()))) & 3
        qb = int(rng.integers(1, L - 25))
        ql = int(rng.integers(19, min(L - qb, 60)))
        if L - qb - ql > 20 and rng.random() < 0.4:   # a deletion from the read to the right of the seed
            c = qb + ql + int(rng.integers(5, L - qb - ql - 5))
            read = np.concatenate([read[:c], read[c + int(rng.integers(1, 9)):]])
            L = len(read)
        if k % 7 == 0:
            read[int(rng.integers(0, L))] = 4
        rb = pos + qb
        w0, w1 = max(lo, pos - margin), min(hi, pos + L + margin)
        win = pacwin.window(pac, L_PAC, w0, w1 - w0)
        read_off, win_off = off, off + L
        pool += [read, win]
        off += L + len(win)
        w = int(rng.choice([100, 100, 30, 7]))
        # left extension (reversed on both sides) and right extension
        tl = rb - w0
        common = dict(qlen=qb, tlen=tl, h0=ql, end_bonus=5, w=w, q_off=read_off + qb - 1)
        for which, t_off, flags in ((0, rb - 1, F.BMH_F_QREV | F.BMH_F_TREV | F.BMH_F_TPAC), (1, win_off + tl - 1, F.BMH_F_QREV | F.BMH_F_TREV)):
            x = np.zeros((), F.EXT_TASK)
            for n_, v_ in common.items():
                x[n_] = v_
            x["t_off"], x["flags"] = t_off, flags
            ext[which].append(x)
        qe = qb + ql
        common = dict(qlen=L - qe, tlen=w1 - (rb + ql), h0=ql + int(rng.integers(0, 40)), end_bonus=5, w=w, q_off=read_off + qe)
        for which, t_off, flags in ((0, rb + ql, F.BMH_F_TPAC), (1, win_off + (rb + ql - w0), 0)):
            x = np.zeros((), F.EXT_TASK)
            for n_, v_ in common.items():
                x[n_] = v_
            x["t_off"], x["flags"] = t_off, flags
            ext[which].append(x)
        # the fused per-seed record over the same window
        for which, t_off, flags in ((0, w0, F.BMH_F_TPAC), (1, win_off, 0)):
            seed[which].append((read_off, t_off, L, qb, ql, rb - w0, w1 - w0, flags, 0))
        # the read against the window, forwards and (every other one) with the window walked down from its last base
        trev = F.BMH_F_TREV if k % 4 >= 2 else 0
        xtra = kswgen.sw_xtra_bwa(P, L)
        sw[0].append((read_off, w1 - 1 if trev else w0, w1 - w0, L, trev | F.BMH_F_TPAC, xtra, 0))
        sw[1].append((read_off, win_off + (w1 - w0 - 1 if trev else 0), w1 - w0, L, trev, xtra, 0))
    pool = np.concatenate(pool + [np.zeros(16, np.uint8)])
    out = dict(pac=pac, pool=pool, ext=[np.array(x) for x in ext], seed=[np.array(x, dtype=F.SEED_TASK) for x in seed],
               sw=[np.array(x, dtype=F.SW_TASK) for x in sw])
    # what the checker says, once; it must agree with itself on the two addressings
    o = {}
    o["ext"] = [kswlib.orc_extend_batch(P, pool, out["ext"][0], nthreads=8, pac=pac, l_pac=L_PAC)[0], kswlib.orc_extend_batch(P, pool, out["ext"][1], nthreads=8)[0]]
    o["seed"] = [kswlib.orc_seedext_batch(P, pool, out["seed"][0], nthreads=8, pac=pac, l_pac=L_PAC)[0], kswlib.orc_seedext_batch(P, pool, out["seed"][1], nthreads=8)[0]]
    o["sw"] = [kswlib.orc_sw_batch(P, pool, out["sw"][0], nthreads=8, pac=pac, l_pac=L_PAC)[0], kswlib.orc_sw_batch(P, pool, out["sw"][1], nthreads=8)[0]]
    for kind in ("ext", "seed"):
        assert (o[kind][0] == o[kind][1]).all(), f"{kind}: the oracle differs between coordinates and pool bytes"
    assert all((o["sw"][0][f] == o["sw"][1][f]).all() for f in kswlib.SW_FIELDS)
    for kind in ("ext", "seed", "sw"):      # both strands, the reverse one past 2^32, the forward one past 2^31
        t = out[kind][0]["t_off"]
        assert (t >= 1 << 32).sum() >= 400 and ((t < L_PAC) & (t >= 1 << 31)).sum() >= 400, kind
    out["want"] = {kind: o[kind][0] for kind in o}
    return out


def _tpac_ctx(tpac, env):
    ctx = _ctx_with(env)
    ctx.set_params(P)
    ctx.set_pac(tpac["pac"], L_PAC)
    return ctx


@pytest.mark.parametrize("mode", ["lane", "lanex4", "reg", "lds"])
def test_tpac_extension_past_2_32(tpac, mode):
    ctx = _tpac_ctx(tpac, {"BMH_EXT_MODE": mode})
    by_pos, by_pool = tpac["ext"]
    dc.assert_ext(ctx.extend_batch(tpac["pool"], by_pos), tpac["want"]["ext"], by_pos, f"{mode}, by coordinate: ")
    dc.assert_ext(ctx.extend_batch(tpac["pool"], by_pool), tpac["want"]["ext"], by_pool, f"{mode}, windows in the pool: ")
    ctx.close()


@pytest.mark.parametrize("mode", ["default", "reg"])
def test_tpac_seedext_past_2_32(tpac, mode):
    ctx = _tpac_ctx(tpac, {} if mode == "default" else {"BMH_EXT_MODE": mode})
    by_pos, by_pool = tpac["seed"]
    dc.assert_seed(ctx.seedext_batch(tpac["pool"], by_pos), tpac["want"]["seed"], by_pos, f"{mode}, by coordinate: ")
    dc.assert_seed(ctx.seedext_batch(tpac["pool"], by_pool), tpac["want"]["seed"], by_pool, f"{mode}, windows in the pool: ")
    ctx.close()


@pytest.mark.parametrize("mode", ["wave", "lane", "generic"])
def test_tpac_sw_past_2_32(tpac, mode):
    ctx = _sw_ctx(mode)
    ctx.set_params(P)
    ctx.set_pac(tpac["pac"], L_PAC)
    by_pos, by_pool = tpac["sw"]
    dc.assert_sw(ctx.sw_batch(tpac["pool"], by_pos), tpac["want"]["sw"], by_pos, f"{mode}, by coordinate: ")
    dc.assert_sw(ctx.sw_batch(tpac["pool"], by_pool), tpac["want"]["sw"], by_pool, f"{mode}, windows in the pool: ")
    ctx.close()
