"""ksw_global2 past the wave kernel's LDS row (bin 4, the band ring), without a GPU: the oracle against the compiled reference on
regions of 10 177-65 535 query columns, the dispatcher model of globallong.py against domaingen's, and the C-ABI of
bmh_global_long_stats.  test_global_long_gpu.py holds the ring kernel to these yardsticks."""
import ctypes as C

import numpy as np
import pytest

import domaingen as dg
import globallong as gl
import kswgen
import kswlib
from __graft_entry__ import load_package

SCORINGS = {"default": dict(), "a2": dict(a=2, b=5, o_del=7, e_del=2, o_ins=5, e_ins=1)}


def test_bounds_follow_the_state_formula():
    assert gl.GLB_LDS_QCAP == 10176 and gl.RING_MAX == 8192 and gl.MAX_RING_W == 4095
    hdr = open(load_package().HEADER_PATH).read()
    assert "10 176" in hdr and "4 095" in hdr


@pytest.mark.ref
@pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built (no reference sources here)")
@pytest.mark.parametrize("scoring", list(SCORINGS))
def test_oracle_global_matches_reference_on_long_regions(scoring):
    rng = np.random.default_rng(7100 + len(scoring))
    p = kswlib.make_params(**SCORINGS[scoring])
    specs = [(10177, 50, "cigar"), (10200, 1, "cigar"), (12000, 200, "tight"), (15000, 800, "cigar"), (21000, 200, "cigar"),
             (33000, 50, "tight"), (40000, 1, "cigar"), (47000, 100, "score"), (65535, 200, "cigar"), (65535, 30, "tight"),
             (11000, 200, "short"), (30000, 50, "short"), (20000, 800, "short")]
    pool, tasks, _ = gl.gen_long(rng, specs)
    assert (tasks["qlen"] > gl.GLB_LDS_QCAP).all()
    assert ((tasks["cigar_cap"] == 0) & (tasks["qlen"].astype(int) > tasks["tlen"].astype(int) + tasks["w"])).sum() == 3
    ref, rcig = kswlib.ref_global_batch(p, pool, tasks)
    orc, ocig = kswlib.orc_global_batch(p, pool, tasks)
    for k in range(len(tasks)):
        assert ref[k] == orc[k] and np.array_equal(rcig[k], ocig[k]), f"task {k} {tasks[k]}: ref={ref[k]} orc={orc[k]}"
    short = tasks["qlen"].astype(int) > tasks["tlen"].astype(int) + tasks["w"]
    assert (ref["score"][short] == -0x40000000).all()  # the untouched initial value of eh[qlen].h (ksw.c:519-522, 565)


def test_route_model_agrees_with_domaingen_without_long_tasks():
    rng = np.random.default_rng(7200)
    for p in (kswlib.make_params(), kswlib.make_params(**SCORINGS["a2"])):
        for k in range(40):
            pool, tasks, _ = kswgen.gen_glb_realistic(rng, int(rng.integers(1, 60)), (int(rng.integers(30, 200)), int(rng.integers(200, 9000))))
            assert (tasks["qlen"] <= gl.GLB_LDS_QCAP).any()
            tasks = tasks[tasks["qlen"] <= gl.GLB_LDS_QCAP]
            if len(tasks) == 0:
                continue
            bins = gl.route(p, tasks)
            assert not (bins == 4).any()
            rows_cap = min(max(1, int(tasks["tlen"].max())), 512)
            assert list(bins) == [dg.glb_lane_bin(p, int(t["qlen"]), int(t["tlen"]), int(t["w"]), rows_cap) for t in tasks]
            assert gl.bin2_lds(tasks) == dg.glb_wave_lds(tasks)


def test_route_model_sends_long_wave_tasks_to_bin_4():
    rng = np.random.default_rng(7300)
    p = kswlib.make_params()
    pool, short, w1 = kswgen.gen_glb_realistic(rng, 30, (100, 150))
    lp, long_, w2 = gl.gen_long(rng, [(10176, 100, "cigar"), (10177, 100, "cigar"), (25000, 5000, "score"), (12000, 40, "score")])
    _, tasks, _ = gl.concat((pool, short, w1), (lp, long_, w2))
    bins = gl.route(p, tasks)
    assert list(bins[30:]) == [2, 4, 4, 4]  # (bin 4 takes a band past the ring too: the kernel refuses it, BMH_E_RANGE)
    assert list(bins[:30]) == list(gl.route(p, short))
    assert gl.long_count(p, tasks) == 3 and gl.long_count(p, tasks, lane_ok=False) == 3
    assert not gl.ring_fits(25000, 5000) and gl.ring_fits(25000, 4095) and gl.ring_fits(3000, 60000)
    # bin 2's variant is chosen from the tasks that fit its row alone
    assert gl.bin2_lds(tasks) == dg.glb_wave_lds(tasks[tasks["qlen"] <= gl.GLB_LDS_QCAP])


def test_global_long_stats_symbol():
    pkg = load_package()
    lib = pkg.lib()
    hdr = open(pkg.HEADER_PATH).read()
    assert "int bmh_global_long_stats(const bmh_ctx_t *ctx, int64_t *tasks, float *ms);" in hdr
    assert hasattr(lib, "bmh_global_long_stats") and "bmh_global_long_stats" in pkg.declared_symbols()
    n, ms = C.c_int64(7), C.c_float(0)
    assert lib.bmh_global_long_stats(None, C.byref(n), C.byref(ms)) == pkg.BMH_E_ARG
    ctx = pkg.Context.__new__(pkg.Context)
    assert callable(ctx.global_long_stats)
