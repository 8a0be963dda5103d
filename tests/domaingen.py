"""Tasks at the edges of the DP kernels' integer domains and routing switches, shared by test_score_domain_cpu.py (oracle vs
the compiled reference) and test_score_domain_gpu.py (kernels vs the oracle).  The routing functions restate, in Python, the
conditions the dispatchers use (ext_bin, glb_wave_lds, sw_bin, sw_kernel_of; the global dispatcher's lane bins are restated once,
in glbbin_ref.py), so that a test can assert that its tasks land on both sides of the switch it targets."""
import numpy as np

import glbband_ref
import glbbin_ref
import kswgen
import kswlib

LIMIT = 32000  # kScoreLimit, bwa-mem-quickassist_amd/csrc/bmh_device.h:22


def max_mat(p):
    return max(0, int(np.max(p["mat"])))  # ksw.c:399-400 starts the maximum at 0


def sw_shift(p):
    return (256 - (int(np.min(p["mat"])) & 0xff)) & 0xff  # ksw_qinit's uint8_t bias, ksw.c:78-85


def big_matrix(rng, a=100, lo=-127):
    """A general (asymmetric) matrix with large entries; the diagonal carries the largest score `a`."""
    m = rng.integers(lo, a // 2, 25).astype(np.int16)
    for i in range(4):
        m[i * 5 + i] = a
    return m.astype(np.int8)


# ---- routing conditions ----------------------------------------------------------------------------------------------

def ext_bin(qlen, mode=0):
    """ext_bin_of, extend_dispatch.hip:26-33 (mode 4 = lanex4; the group-kernel tlen switch is left out)."""
    if mode == 1 or qlen < 1:
        return 5
    return 0 if qlen <= 32 else 1 if qlen <= 64 else 2 if qlen <= 128 else 3 if qlen <= 256 else 4 if (qlen <= 512 and mode == 4) else 5


def glb_lane_bin(p, qlen, tlen, w, rows_cap, c32=0, exact=0):
    """The kernel class of a task on band w, from glbband_ref.lane_domain and glbbin_ref.lane_bin: 0/3/1 = the lane kernels' domain at
    bands up to 31/47/63, 2 = the int32 wave kernel.  c32 and exact switch on the dispatcher's narrower bins 5, 6 and 7, which split
    class 0 further (glbbin_ref.expected_bins gives a whole batch's bins, with the band pass as well)."""
    return glbbin_ref.lane_bin(w, c32, exact) if glbband_ref.lane_domain(p, qlen, tlen, w, rows_cap) else 2


def glb_wave_lds(tasks):
    """Which variant of global_kernel a batch's wave-kernel tasks take (global_kernel.hip:281-288, from validate_glb's
    qmax / tmax / wmax, api.hip:728-729): True = direction bytes in LDS, False = HBM scratch.  One choice per batch."""
    qmax, tmax = max(1, int(tasks["qlen"].max())), max(1, int(tasks["tlen"].max()))
    wmax = max(0, int(np.minimum(tasks["w"], tasks["qlen"].astype(np.int64)).max()))
    qcap = (qmax + 63) & ~63
    state = 8 * (qcap + 2) + 8 * qcap + 32
    ncol = qmax if qmax < 2 * wmax + 1 else 2 * wmax + 1
    zcap = max(16, (ncol * tmax + 15) & ~15)
    return state + zcap <= 64 * 1024


def glb_worst(p, qlen, tlen):
    emax = max(int(p["e_del"]), int(p["e_ins"]))
    smax = max(max(0, -int(np.min(p["mat"]))), max_mat(p))
    return int(p["o_del"]) + int(p["o_ins"]) + emax * (qlen + tlen) + smax * max(qlen, tlen)


def sw_bin(p, qlen, xtra):
    """sw_bin_of, sw_dispatch.hip:32-42: 0/1/6 byte-mode register bins (80/160/256 padded columns), 7 word-mode register
    bin, 2 the slab kernel."""
    mx, sh = max_mat(p), sw_shift(p)
    if qlen < 1:
        return 2
    if not xtra & kswlib.KSW_XBYTE:
        half = ((((qlen + 7) >> 3) * 4) + 7) & ~7
        return 7 if half <= 128 and qlen * mx + sh < 512 else 2
    if qlen * mx + sh >= 255:
        return 2
    qp = (qlen + 15) // 16 * 16
    return 0 if qp <= 80 else 1 if qp <= 160 else 6 if qp <= 256 else 2


def sw_wave_fits(tasks):
    """sw_wave_fits, sw_wave.hip:190-193: a batch of up to 32 768 tasks whose padded longest query is at most 320 columns
    (and longest target at most 16 384 rows) goes to sw_wave_kernel on the default path (launch_sw, sw_dispatch.hip)."""
    q = (max(1, int(tasks["qlen"].max())) + 15) // 16 * 16
    return 0 < len(tasks) <= 32768 and q <= 320 and int(tasks["tlen"].max()) <= 16384


def sw_wave_takes(p, qlen, xtra, max_cols):
    """sw_wave_takes, sw_common.h:45-50: the tasks sw_wave_kernel computes; the rest of its batch goes to the slab kernel."""
    segs = 16 if xtra & kswlib.KSW_XBYTE else 8
    if qlen < 1 or (qlen + segs - 1) // segs * segs > max_cols:
        return False
    return qlen * max_mat(p) + sw_shift(p) < (255 if xtra & kswlib.KSW_XBYTE else 512)


def sw_kernel_of(p, tasks, mode):
    """The kernel launch_sw (sw_dispatch.hip) gives each task of a batch under the test's modes: 'wave' (the default path),
    'lane' (BMH_SW_WAVE=0) or 'generic' (BMH_SW_MODE=generic).  Returns 'wave', 'generic' or the register bin number."""
    if mode == "generic":
        return ["generic"] * len(tasks)
    qmax = max(1, int(tasks["qlen"].max()))
    if mode == "wave" and sw_wave_fits(tasks):
        cols = 192 if (qmax + 15) // 16 * 16 <= 192 else 320
        return ["wave" if sw_wave_takes(p, int(t["qlen"]), int(t["xtra"]), cols) else "generic" for t in tasks]
    out = []
    for t in tasks:
        b = sw_bin(p, int(t["qlen"]), int(t["xtra"]))
        if b == 2:  # the slab kernel's bin; past 256 columns the default path hands what fits 320 columns to sw_wave_kernel
            wave = mode == "wave" and qmax > 256 and int(tasks["tlen"].max()) <= 16384 and sw_wave_takes(p, int(t["qlen"]), int(t["xtra"]), 320)
            b = "wave" if wave else "generic"
        out.append(b)
    return out


# ---- sequences --------------------------------------------------------------------------------------------------------

def related(rng, qlen, tlen, sub=0.01, indel=0.0, max_indel=1, early_indel=False):
    """A query and a target that starts with a mutated copy of it; `early_indel` puts one indel a few bases in, so that a
    gap penalty that is read wrong changes the best alignment."""
    q = kswgen.rand_seq(rng, qlen)
    t = kswgen.mutate(rng, q, sub, indel, indel, max_indel)
    if early_indel and qlen > 12:
        k = int(rng.integers(3, 8))
        t = np.concatenate([t[:k], kswgen.rand_seq(rng, int(rng.integers(1, 4))), t[k:]]) if rng.random() < 0.5 else np.concatenate([t[:k], t[k + int(rng.integers(1, 4)):]])
    t = np.concatenate([t, kswgen.rand_seq(rng, max(0, tlen - len(t)))])[:tlen]
    return q, t.astype(np.uint8)


# ---- extension (ksw_extend2) ------------------------------------------------------------------------------------------

EXT_QLENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)


def gen_ext_edges(rng, p, qlens=EXT_QLENS, per=4, long_q=0, early_indel=False):
    """Extension tasks whose h0 + qlen*max(mat) is exactly 32000, 31999 and spread below, at every bin edge +-1 the matrix
    allows, with bands and end bonuses up to 32767; `long_q` adds one task of that query length (the LDS kernel)."""
    mx = max(1, max_mat(p))
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    lens = [q for q in qlens if q * mx <= LIMIT] + ([long_q] if long_q and long_q * mx <= LIMIT else [])
    for qlen in lens:
        room = LIMIT - qlen * mx
        for k in range(per):
            h0 = [room, room - 1, int(rng.integers(0, room + 1)), room // 2][k % 4]
            if h0 < 0:
                continue
            gap = int(rng.integers(0, 40)) if qlen < 2000 else 200
            q, t = related(rng, qlen, min(65535, qlen + gap), sub=float(rng.choice([0.0, 0.01, 0.05])),
                           indel=float(rng.choice([0.0, 0.005, 0.02])), max_indel=3, early_indel=early_indel)
            w = int(rng.choice([1, 10, 100, 1000, 32767]))
            eb = int(rng.choice([0, 5, 1000, 32767]))
            kswgen._add_ext(pb, rng, q, t, h0, w, eb)
    return pb.finish()


def ext_edge_param_sets(rng):
    """Scaled matrices (a and b up to 127, general matrices) and gap costs past 2^15 and 2^16, symmetric and not."""
    g = big_matrix(rng, 100)
    return [
        kswlib.make_params(a=60, b=127, o_del=100, e_del=30, o_ins=100, e_ins=30, zdrop=30000),
        kswlib.make_params(a=127, b=127, o_del=127, e_del=127, o_ins=127, e_ins=127, zdrop=-1),
        kswlib.make_params(a=20, b=60, o_del=200, e_del=40, o_ins=150, e_ins=50, zdrop=0),
        kswlib.make_params(a=64, mat=g, o_del=90, e_del=20, o_ins=60, e_ins=25, zdrop=500),
        kswlib.make_params(a=20, b=30, o_del=40000, e_del=1, o_ins=6, e_ins=1),
        kswlib.make_params(a=20, b=30, o_del=70000, e_del=1, o_ins=70000, e_ins=1, zdrop=30000),
        kswlib.make_params(a=20, b=30, o_del=6, e_del=1, o_ins=65535, e_ins=2),
        kswlib.make_params(a=20, b=30, o_del=0, e_del=65537, o_ins=0, e_ins=65537, zdrop=-1),
        kswlib.make_params(a=20, b=30, o_del=40000, e_del=30000, o_ins=6, e_ins=1),
        kswlib.make_params(a=20, b=30, o_del=65534, e_del=1, o_ins=6, e_ins=1),
        kswlib.make_params(a=20, b=30, o_del=0, e_del=65535, o_ins=0, e_ins=65535, zdrop=-1),
        kswlib.make_params(a=20, b=30, o_del=0, e_del=16383, o_ins=0, e_ins=16383, zdrop=-1),
        kswlib.make_params(a=20, b=30, o_del=49152, e_del=16383, o_ins=30000, e_ins=16383),
        kswlib.make_params(a=20, b=30, o_del=6, e_del=1, o_ins=0, e_ins=16384),
    ]


def ext_gaps_accepted(p):
    """bmh_extend_batch / bmh_seedext_batch take o+e <= 65535 and e <= 16383 on either side (bmh_ctx.h, ext_gaps_too_large)."""
    return (int(p["o_del"]) + int(p["e_del"]) <= 65535 and int(p["o_ins"]) + int(p["e_ins"]) <= 65535
            and int(p["e_del"]) <= 16383 and int(p["e_ins"]) <= 16383)


# ---- global (ksw_global2) ---------------------------------------------------------------------------------------------

def _add_glb(pb, rng, qlen, tlen, w):
    q, t = related(rng, qlen, tlen, sub=0.03, indel=0.01, max_indel=4)
    if len(t) < tlen:
        t = np.concatenate([t, kswgen.rand_seq(rng, tlen - len(t))])
    kswgen._add_glb(pb, q, t[:tlen], w)


def gen_glb_worst_edges(rng, p, per=6):
    """Tasks whose |score| bound `worst` (global_kernel.hip:231) is exactly 11999 and 12000, and some around them, all with
    tlen <= 512 and bands <= 63 (so that `worst` alone decides between the lane and the wave kernels)."""
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for target in (11999, 12000, 11995, 12005):
        hits = [(q, t) for t in range(8, 513) for q in range(max(1, t - 60), t + 61) if glb_worst(p, q, t) == target]
        assert hits, f"no task shape has worst = {target} under these parameters"
        for k in rng.choice(len(hits), size=per if target in (11999, 12000) else 2):
            q, t = hits[int(k)]
            _add_glb(pb, rng, q, t, min(63, abs(t - q) + int(rng.integers(0, 18))))
    return kswgen.finish_glb(pb)


def gen_glb_shape_edges(rng, per=4):
    """tlen 512/513 (the lane kernels' slab, global_kernel.hip:256) and bands 31/32, 47/48, 63/64."""
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for tlen in (511, 512, 513, 600):
        for _ in range(per):
            _add_glb(pb, rng, tlen - int(rng.integers(0, 20)), tlen, int(rng.choice([20, 31, 40, 63])))
    for w in (31, 32, 47, 48, 63, 64):
        for _ in range(per):
            qlen = int(rng.integers(60, 300))
            tlen = qlen + int(rng.integers(-min(w, 20), min(w, 20) + 1))
            _add_glb(pb, rng, qlen, max(1, tlen), w)
    return kswgen.finish_glb(pb)


def gen_glb_deep(rng, lens=(300, 1200), per=4):
    """Long divergent pairs under a scaled matrix: scores far into the int32 range, in the wave kernel's LDS (300) and HBM
    scratch (1200) variants."""
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for L in lens:
        for _ in range(per):
            q = kswgen.rand_seq(rng, L)
            t = kswgen.mutate(rng, q, 0.3, 0.03, 0.03, 20)
            if rng.random() < 0.5:
                t = kswgen.rand_seq(rng, L + int(rng.integers(-30, 30)))
            kswgen._add_glb(pb, q, t, abs(len(q) - len(t)) + int(rng.integers(5, 80)))
    return kswgen.finish_glb(pb)


# ---- global: real scores across the lane kernels' 16-bit domain ---------------------------------------------------------
# Every family below yields (label, params, (pool, tasks, cigar words)) batches, one per scoring, whose tasks ALL satisfy
# glbband_ref.lane_domain (asserted in _lane_batch): none can drift to the int32 wave kernel.  No task has tlen > qlen + w, where
# the reference's traceback is undefined.

MINUS_INF = -0x40000000  # ksw.c:487
GLB_LANE_BINS = (6, 7, 5, 0, 3, 1)


def _lane_batch(p, pb):
    pool, tasks, words = kswgen.finish_glb(pb)
    assert len(tasks)
    rows_cap = min(int(tasks["tlen"].max()), glbband_ref.ROWS_CAP)
    for t in tasks:
        assert glbband_ref.lane_domain(p, int(t["qlen"]), int(t["tlen"]), int(t["w"]), rows_cap), f"outside the lane domain: {t}"
        assert int(t["tlen"]) <= int(t["qlen"]) + int(t["w"]), f"tlen > qlen + w: {t}"
    return pool, tasks, words


def _in_domain(p, ql, tl):
    return tl <= glbband_ref.ROWS_CAP and glb_worst(p, ql, tl) < 12000 and int(p["o_del"]) + int(p["o_ins"]) < 4000


def _disjoint(rng, ql, tl):
    """A query over codes {0,1} and a target over {2,3}: every cell is a mismatch."""
    return rng.integers(0, 2, ql).astype(np.uint8), rng.integers(2, 4, tl).astype(np.uint8)


DEEP_GAPS = ((60, 4, 60, 4), (1000, 4, 1000, 4), (1800, 1, 1800, 1), (3000, 1, 600, 1), (600, 1, 3000, 1))
DEEP_BANDS = (0, 1, 2, 3, 4, 5, 7, 8, 12, 15)


def gen_glb_deep_negative_equal(rng):
    """b = 64, 100, 127 on all-mismatch pairs of 64..90 bases (the longest the domain admits under each scoring, and a few below) at
    own bands 0..15, tlen = qlen, qlen +- 1, qlen +- 3 (qlen - tlen > w: the reference's MINUS_INF)."""
    out = []
    for b in (64, 100, 127):
        for od, ed, oi, ei in DEEP_GAPS:
            p = kswlib.make_params(a=1, b=b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei)
            top = max(L for L in range(64, 91) if _in_domain(p, L, L))  # (64 is inside under every one of these scorings)
            pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
            for k, w in enumerate(DEEP_BANDS):
                for d in (0, 1, -1, 3, -3):  # tlen - qlen
                    ql = max(64, top - (k + abs(d)) % 3 - max(d, 0))
                    tl = ql + d
                    if tl > ql + w or not _in_domain(p, ql, tl):
                        continue
                    q, t = _disjoint(rng, ql, tl)
                    kswgen._add_glb(pb, q, t, w, want_cigar=(k + d) % 5 != 0)
            out.append((f"b={b} gaps={(od, ed, oi, ei)}", p, _lane_batch(p, pb)))
    return out


def gen_glb_threshold():
    """A^L against C^L, L = 127, 128, 129 under a=1 b=64: scores -8128, -8192, -8256, either side of half the -16384 sentinel.  At
    w = 0 under the default gaps; at w = 5 and 12 under gap opens large enough that the all-mismatch diagonal stays the optimum.
    o_del = o_ins = 1900 puts all three lengths outside the domain (worst = 12182, 12248, 12314); 1740 is the largest open that
    keeps L = 129 inside (worst = 11994), so the three run under that."""
    out = []
    for label, o, bands in (("o=6", 6, (0,)), ("o=1740", 1740, (0, 5, 12))):
        p = kswlib.make_params(a=1, b=64, o_del=o, e_del=1, o_ins=o, e_ins=1)
        assert not any(_in_domain(kswlib.make_params(a=1, b=64, o_del=1900, e_del=1, o_ins=1900, e_ins=1), L, L) for L in (127, 128, 129))
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        for w in bands:
            for L in (127, 128, 129):
                kswgen._add_glb(pb, np.zeros(L, np.uint8), np.ones(L, np.uint8), w)
        out.append((f"threshold {label}", p, _lane_batch(p, pb)))
    return out


# (b, o_del, o_ins, e).  The last three go deeper in the wide bins: a smaller mismatch cost admits longer pairs (251 and 366 rows), and
# with b*d < min(o_del, o_ins) + 2d a second gap inside the band never pays, so the score stays -(b*min(qlen,tlen) + o + e*d).
UNEQUAL_SCORINGS = ((60, 999, 3000, 1), (60, 3000, 999, 1), (80, 500, 2500, 1), (90, 1999, 2000, 1),
                    (30, 999, 3000, 1), (30, 3000, 999, 1), (20, 999, 3000, 1))
UNEQUAL_DELTAS = (16, 20, 24, 31, 32, 40, 47, 48, 56, 63)


def gen_glb_deep_negative_unequal(rng):
    """Disjoint alphabets with |qlen - tlen| = d and w = d + 0, 1, 2 (<= 63), both signs, at the longest lengths the domain admits."""
    out = []
    for b, od, oi, e in UNEQUAL_SCORINGS:
        p = kswlib.make_params(a=1, b=b, o_del=od, e_del=e, o_ins=oi, e_ins=e)
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        for d in UNEQUAL_DELTAS:
            top = max(L for L in range(d + 1, 513) if _in_domain(p, L, L - d))
            for slack in (0, 1, 2):
                if d + slack > 63:
                    continue
                for ql, tl in ((top, top - d), (top - d, top)):  # an insertion of d bases, a deletion of d bases
                    q, t = _disjoint(rng, ql, tl)
                    kswgen._add_glb(pb, q, t, d + slack, want_cigar=slack != 1 or ql > tl)
        out.append((f"unequal b={b} gaps={(od, e, oi, e)}", p, _lane_batch(p, pb)))
    return out


EMPTY_BANDS = (0, 2, 3, 7, 12, 20, 40, 47, 60, 63)


def gen_glb_empty_target(rng):
    """tlen = 0: the score is eh[qlen].h of ksw.c:519-522, -(o_ins + e_ins*qlen) for qlen <= w and MINUS_INF past the band.  Per band
    one scoring with o_ins = 3000 and the smallest e_ins that takes qlen = w to -8192 or below (qlen = w + 1 is then still inside the
    domain); and every shape once under the default gaps."""
    out = []
    shapes = [(w, ql) for w in EMPTY_BANDS for ql in sorted({w, w + 1, 1, 3})]
    for w in EMPTY_BANDS:
        e = -(-(8192 - 3000) // w) if w else 1
        p = kswlib.make_params(o_del=6, e_del=1, o_ins=3000, e_ins=e)
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        for ww, ql in shapes:
            if ww == w:
                kswgen._add_glb(pb, kswgen.rand_seq(rng, ql), np.zeros(0, np.uint8), w, want_cigar=ql != 3)
        out.append((f"empty target w={w} e_ins={e}", p, _lane_batch(p, pb)))
    p = kswlib.make_params()
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for w, ql in shapes:
        kswgen._add_glb(pb, kswgen.rand_seq(rng, ql), np.zeros(0, np.uint8), w)
    out.append(("empty target, default gaps", p, _lane_batch(p, pb)))
    return out


POSITIVE_BANDS = (0, 3, 7, 15, 31, 47, 63)


def gen_glb_deep_positive(rng):
    """Identical sequences: a=127 b=127 on 80, 90 and 92 bases (10160 .. 11684), a=21 b=21 on 500 bases (10500)."""
    out = []
    p = kswlib.make_params(a=127, b=127)
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for L in (80, 90, 92):
        for w in POSITIVE_BANDS:
            q = kswgen.rand_seq(rng, L)
            kswgen._add_glb(pb, q, q.copy(), w)
    out.append(("a=127", p, _lane_batch(p, pb)))
    p = kswlib.make_params(a=21, b=21)
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for w in (0, 7):
        q = kswgen.rand_seq(rng, 500)
        kswgen._add_glb(pb, q, q.copy(), w)
    out.append(("a=21, 500 bases", p, _lane_batch(p, pb)))
    return out


EXTREME_GAPS = ((6, 1150, 6, 1150), (6, 1150, 6, 3), (3, 2, 6, 1150), (2000, 1, 1999, 1))


def gen_glb_extreme_gaps():
    """Every pair of up to five bases of two letters at every band up to 7 (26 576 tasks) under gap extensions of 1150 and gap opens of
    1999 + 2000, all inside the domain; and the 11 216 of them that a=100 b=127 with gaps (1999, 900, 2000, 900) leaves inside."""
    pool, tasks, _ = glbband_ref.exhaustive_set(2, 5, 7)
    out = []
    for od, ed, oi, ei in EXTREME_GAPS:
        p = kswlib.make_params(o_del=od, e_del=ed, o_ins=oi, e_ins=ei)
        out.append((f"exhaustive gaps={(od, ed, oi, ei)}", p, _lane_subset(p, pool, tasks)))
        assert len(out[-1][2][1]) == 26576
    p = kswlib.make_params(a=100, b=127, o_del=1999, e_del=900, o_ins=2000, e_ins=900)
    out.append(("exhaustive a=100 b=127 gaps=(1999, 900, 2000, 900)", p, _lane_subset(p, pool, tasks)))
    assert len(out[-1][2][1]) == 11216
    return out


def _lane_subset(p, pool, tasks):
    """The tasks inside the lane domain (judged with the slab of the whole set: no target here is longer), CIGAR offsets re-packed."""
    keep = np.array([_in_domain(p, int(t["qlen"]), int(t["tlen"])) for t in tasks])
    sub = tasks[keep].copy()
    sub["cigar_off"] = np.cumsum(sub["cigar_cap"]) - sub["cigar_cap"]
    return pool, sub, int(sub["cigar_cap"].sum())


def n_matrix(rng, a, lo):
    """big_matrix with nine distinct entries in row 4 and column 4 (the N base), none equal to a regular entry of its row or column:
    a selector that reads another base for N, or N for "no base", changes the score."""
    while True:
        m = big_matrix(rng, a, lo).astype(np.int64).reshape(5, 5)
        edge = np.concatenate([m[4, :], m[:4, 4]])
        if len(set(edge.tolist())) == 9 and all(m[4, j] not in m[:4, j] and m[i, 4] not in m[i, :4] for i in range(4) for j in range(4)):
            return m.reshape(25).astype(np.int8)


N_BANDS = (0, 1, 2, 3, 4, 5, 6, 7, 12)


def gen_glb_n_bases(rng, per=6):
    """Queries of 20..90 bases with 15 % N against mutated copies at own bands 0..7 and 12, under general matrices with entries down
    to -120 (a = 100; with gap costs (40, 3, 30, 4) a pair of 90 bases has worst = 11590) and to -60 (a = 50, default gaps)."""
    out = []
    for a, lo, gaps in ((100, -120, dict(o_del=40, e_del=3, o_ins=30, e_ins=4)), (50, -60, dict())):
        p = kswlib.make_params(a=a, mat=n_matrix(rng, a, lo), **gaps)
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        for w in N_BANDS:
            for k in range(per):
                ql = (20, 90)[k] if k < 2 else int(rng.integers(20, 91))
                q = kswgen.rand_seq(rng, ql, p_n=0.15)
                t = kswgen.mutate(rng, q, 0.1, 0.03 if w else 0.0, 0.03 if w else 0.0, 3)
                t[rng.random(len(t)) < 0.05] = 4
                tl = int(np.clip(len(t), max(1, ql - w), min(ql + w, 90)))
                t = np.concatenate([t, kswgen.rand_seq(rng, max(0, tl - len(t)), p_n=0.15)])[:tl]
                kswgen._add_glb(pb, q, t.astype(np.uint8), w, want_cigar=k != 3)
        out.append((f"N bases a={a}", p, _lane_batch(p, pb)))
    return out


# ---- local Smith-Waterman (ksw_align2) --------------------------------------------------------------------------------

X_START = kswlib.KSW_XSUBO | kswlib.KSW_XSTART
X_SCORE = kswlib.KSW_XSUBO  # no start positions: with byte overflow the reference defines only the score (ksw.c:198-200)


def sw_task(pb, rng, qlen, tlen, xtra, sub=0.02):
    """A query and a window holding a mutated copy of it somewhere inside."""
    t = kswgen.rand_seq(rng, tlen)
    q = kswgen.rand_seq(rng, qlen)
    if tlen > 8 and rng.random() < 0.85:
        st = int(rng.integers(0, max(1, tlen - qlen // 2)))
        core = kswgen.mutate(rng, t[st:st + qlen], sub, 0.005, 0.005, 3)
        q = np.concatenate([core, kswgen.rand_seq(rng, max(0, qlen - len(core)))])[:qlen]
    kswgen._add_sw(pb, rng, q.astype(np.uint8), t, xtra)


def gen_sw_edges(rng, p, cases, per=3):
    """cases: (qlen, xtra) pairs; each becomes `per` tasks against windows of qlen + 20 .. qlen + 400 bases."""
    pb = kswgen.PoolBuilder(kswlib.SW_TASK)
    for qlen, xtra in cases:
        for _ in range(per):
            sw_task(pb, rng, qlen, qlen + int(rng.integers(20, 400)), xtra | (19 * max(1, max_mat(p))))
    return pb.finish()


def sw_edge_cases(p):
    """Routing edges the matrix of `p` reaches: byte mode qlen*max + shift = 254 / 255 (ksw_u8 overflow, sw_dispatch.hip:39),
    word mode < 512 (sw_dispatch.hip:37), padded queries of 80/81, 160/161, 256/257 columns."""
    mx, sh = max(1, max_mat(p)), sw_shift(p)
    B = kswlib.KSW_XBYTE
    out = []
    for s in (253, 254, 255, 256):  # byte overflow edge
        q = (s - sh) // mx
        if q >= 1:
            out.append((q, B | (X_START if q * mx + sh < 255 else X_SCORE)))
    for s in (510, 511, 512):  # word register bin
        q = (s - sh) // mx
        if q >= 1:
            out.append((q, X_START))
    for q in (80, 81, 96, 97, 160, 161, 176, 192, 193, 256, 257, 320, 321):
        if q * mx + sh < 255:
            out.append((q, B | X_START))
        out.append((q, X_START))
    for q in (1, 2, 15, 16, 17):
        out.append((q, B | (X_START if q * mx + sh < 255 else X_SCORE)))
        out.append((q, 0))
    return [(q, x) for q, x in out if q * mx < LIMIT]  # bmh_sw_batch's accepted range (api.hip:896)


def sw_gap_param_sets():
    """Gap costs up to 255 (bmh_sw_batch's limit); the first five wrap o+e in ksw_u8's 8-bit lanes."""
    wrap = [(128, 128, 1, 1), (1, 1, 128, 128), (130, 127, 130, 127), (130, 127, 1, 128), (250, 10, 3, 250)]
    fine = [(100, 100, 100, 100), (200, 55, 250, 5), (120, 1, 1, 1), (1, 254, 254, 1), (0, 1, 254, 1)]
    return [(g, True) for g in wrap] + [(g, False) for g in fine]


def wraps(p):
    return int(p["o_del"]) + int(p["e_del"]) > 255 or int(p["o_ins"]) + int(p["e_ins"]) > 255
