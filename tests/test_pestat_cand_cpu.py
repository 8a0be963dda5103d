"""mem_pestat in two halves, on the CPU: bmh_pestat_candidates (the pair walk, host/pestat_core.h) and bmh_pestat_from_candidates
(the statistics) against
 * the compiled reference's mem_pestat table -- the pairing groups of tests/golden/orient_golden.npz, the pairs of
   postproc_golden.npz and, where oracle/_ref is built, further seeds live -- and bmh_pestat's table on all of these, bit for bit;
 * a plain Python restatement of bwamem_pair.c:23-62 (tests/pestat_ref.py), word for word, on those and on hand-made vectors for
   every exit and edge of the rule (that each class occurs is counted from the restatement alone);
 * the finish at its own edges, against bmh_pestat on vectors that yield the same candidates;
 * tests/pestat_core_main.c, the core as a stand-alone program, plainly and under AddressSanitizer with every slice in a heap block
   of its exact size: its digest of the words against the library's words."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import kswlib
import orientgen as og
import pestat_ref as pr
import postgen
from __graft_entry__ import load_package
from test_postproc_cpu import L, sam_opt, split  # noqa: F401  (L: the module-scoped fixture)

ROOT = kswlib.ROOT
PAIR_KEYS = [f"p{si}_{mix}_" for si in (0, 2) for mix in og.MIXES]
SRC = os.path.join(ROOT, "tests", "pestat_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
FIELDS = ("low", "high", "failed", "avg", "std")
L_PAC = 3_000_000


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def bits(pes):
    return [np.ascontiguousarray(pes[f]).view(np.uint32 if pes[f].dtype.itemsize == 4 else np.uint64).tolist() for f in FIELDS]


def whole(L, o, vecs, l_pac, verbose=-1):  # noqa: N803
    c_regs = kswlib.regs_to_c(vecs)
    pes = np.zeros(4, dtype=kswlib.PESTAT)
    L.bmh_pestat(o.ctypes.data_as(C.c_void_p), C.c_int64(l_pac), len(vecs), c_regs, pes.ctypes.data_as(C.c_void_p), verbose)
    kswlib.regs_from_c(c_regs)
    return pes


def halves(pkg, o, vecs, l_pac, verbose=-1):
    w = pkg.pestat_candidates(o, l_pac, vecs)
    return w, pkg.pestat_from_candidates(o, w, verbose)


def check_group(pkg, L, o, vecs, l_pac, want_pes=None, restate=True):  # noqa: N803
    w, pes = halves(pkg, o, vecs, l_pac)
    assert bits(pes) == bits(whole(L, o, vecs, l_pac))
    if want_pes is not None:
        assert bits(pes) == bits(want_pes), (pes, want_pes)
    if restate:
        want_w, seen = pr.words(o, l_pac, vecs)
        assert (w == want_w).all(), np.nonzero(w != want_w)[0][:5]
        return w, seen
    return w, {}


# ---------------------------------------------------------------- against the reference's table, bmh_pestat and the restatement

@pytest.mark.parametrize("key", PAIR_KEYS)
def test_orient_fixture_groups(pkg, L, key):  # noqa: F811
    _, si, _, l_pac, vecs, _, want_pes, _ = og.pairing_group(key)
    w, seen = check_group(pkg, L, sam_opt(**postgen.OPTION_SETS[si]), vecs, l_pac, want_pes)
    assert (w != 0).sum() > 100
    if "_all4_" in key:
        assert all(seen.get(f"dir{d}", 0) >= 10 for d in range(4)), seen


def test_postproc_fixture_pairs(pkg, L):  # noqa: F811
    g = np.load(os.path.join(kswlib.GOLDEN_DIR, "postproc_golden.npz"))
    for si, kw in enumerate(postgen.OPTION_SETS):
        p = f"s{si}_"
        w, _ = check_group(pkg, L, sam_opt(**kw), split(g[p + "pairs"], g[p + "pairs_off"]), 1_000_000, g[p + "pes"])
        assert (w != 0).sum() > 30


@pytest.mark.ref
@pytest.mark.parametrize("seed", [3, 4])
def test_live_reference_on_further_seeds(pkg, L, seed):  # noqa: F811
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_orient_fixture as mk
    for si in range(len(postgen.OPTION_SETS)):
        for mi, mix in enumerate(og.MIXES.values()):
            vecs, _ = og.paired_vectors4(np.random.default_rng(7000 + 100 * seed + 10 * si + mi), 400, L_PAC, mix)
            want_pes, _ = mk.ref_pairing(reflib.lib(), postgen.OPTION_SETS[si], vecs, L_PAC)
            check_group(pkg, L, sam_opt(**postgen.OPTION_SETS[si]), vecs, L_PAC, want_pes, restate=(seed == 3 and si in (0, 3)))


def test_stderr_text_is_the_same(pkg, L, capfd):  # noqa: F811
    _, si, _, l_pac, vecs, _, _, _ = og.pairing_group("p0_all4_")
    o = sam_opt(**postgen.OPTION_SETS[si])
    capfd.readouterr()
    whole(L, o, vecs, l_pac, verbose=3)
    one = capfd.readouterr().err
    halves(pkg, o, vecs, l_pac, verbose=3)
    two = capfd.readouterr().err
    assert one == two and one.count("[M::mem_pestat]") >= 10, (one, two)


# ---------------------------------------------------------------- hand-made vectors: every exit and edge of the rule

@pytest.mark.parametrize("kw", [dict(), dict(max_ins=600, min_seed_len=25), dict(a=2, b=8, mask_level=0.25)])
def test_handmade_vectors_reach_every_class(pkg, L, kw):  # noqa: F811
    o = sam_opt(**kw)
    vecs = pr.handmade(o, L_PAC)
    w, seen = check_group(pkg, L, o, vecs, L_PAC)
    print(seen)
    missing = [t for t in pr.ALL_TAGS if not seen.get(t)]
    assert not missing, missing
    assert max(len(v) for v in vecs) == 40
    dirs = w[w != 0] >> 30
    assert set(dirs.tolist()) == {0, 1, 2, 3}
    # the edges decide: at 0.8 * score a candidate, one above none; max_ins in, max_ins + 1 out
    for p in range(len(w)):
        _, tags = pr.word(o, L_PAC, vecs[2 * p], vecs[2 * p + 1])
        if tags & {"sub0_above", "sub1_above", "is0", "is_max1", "empty0", "empty1"}:
            assert w[p] == 0, (p, tags)
        if "is_max" in tags and not tags & {"sub0_reject", "sub1_reject"}:
            assert w[p] & 0x3fffffff == int(o["max_ins"])


def test_arguments(pkg):
    o = sam_opt()
    lib = pkg.lib()
    v = kswlib.regs_to_c(pr.pair_of(L_PAC, 1, 300))
    w = np.zeros(1, dtype=np.uint32)
    pes = np.full(4, 7, dtype=kswlib.PESTAT)
    op, wp, pp = o.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), pes.ctypes.data_as(C.c_void_p)
    E_ARG, E_RANGE = -3, -4
    assert lib.bmh_pestat_candidates(None, L_PAC, 2, v, wp) == E_ARG
    assert lib.bmh_pestat_candidates(op, L_PAC, 2, None, wp) == E_ARG
    assert lib.bmh_pestat_candidates(op, L_PAC, 2, v, None) == E_ARG
    assert lib.bmh_pestat_candidates(op, L_PAC, -1, v, wp) == E_ARG
    assert lib.bmh_pestat_candidates(op, L_PAC, 2, v, wp) == 0 and w[0] == (1 << 30 | 300)
    w[0] = 0xdead
    assert lib.bmh_pestat_candidates(op, L_PAC, 1, v, wp) == 0 and w[0] == 0xdead  # an odd n ignores the last read
    assert lib.bmh_pestat_from_candidates(None, 1, wp, pp, -1) == E_ARG
    assert lib.bmh_pestat_from_candidates(op, 1, None, pp, -1) == E_ARG
    assert lib.bmh_pestat_from_candidates(op, 1, wp, None, -1) == E_ARG
    assert lib.bmh_pestat_from_candidates(op, -1, wp, pp, -1) == E_ARG
    for bad in (1 << 30, 3 << 30, int(o["max_ins"]) + 1, 2 << 30 | (int(o["max_ins"]) + 1)):  # is == 0, is > max_ins
        ws = np.array([1 << 30 | 300, bad], dtype=np.uint32)
        assert lib.bmh_pestat_from_candidates(op, 2, ws.ctypes.data_as(C.c_void_p), pp, -1) == E_ARG
    assert (pes == np.full(4, 7, dtype=kswlib.PESTAT)).all()  # refused: pes untouched
    big = sam_opt(max_ins=1 << 30)
    bp = big.ctypes.data_as(C.c_void_p)
    assert lib.bmh_pestat_candidates(bp, L_PAC, 2, v, wp) == E_RANGE
    assert lib.bmh_pestat_from_candidates(bp, 1, wp, pp, -1) == E_RANGE
    assert lib.bmh_pestat_from_candidates(op, 0, None, pp, -1) == 0 and (pes["failed"] == 1).all()
    kswlib.regs_from_c(v)


def test_host_only_pestat_keeps_serving_a_huge_max_ins(L):  # noqa: F811
    o = sam_opt(max_ins=(1 << 31) - 1)
    big_pac = 1 << 40
    vecs = []
    for k in range(12):
        vecs += pr.pair_of(big_pac, 1, (1 << 30) + 1000 + k, b1=1 << 20)
    pes = whole(L, o, vecs, big_pac)
    assert list(pes["failed"]) == [1, 0, 1, 1] and (1 << 30) + 1000 <= pes["avg"][1] <= (1 << 30) + 1011


# ---------------------------------------------------------------- the finish at its own edges

def _vectors_for(cands):
    """one-region vectors whose candidates are exactly `cands`: (orientation, insert size) per pair"""
    c = np.asarray(cands, dtype=np.int64).reshape(-1, 2)
    d, dist = c[:, 0], c[:, 1]
    flat = np.repeat(pr.reg(0), 2 * len(c))
    b1 = L_PAC // 2 + L_PAC * (np.arange(len(c)) & 1)  # mate 1 on either strand
    p2 = np.where(d <= 1, b1 + dist, b1 - dist)  # pestat_ref.mate_rb, for arrays
    flat["rb"][0::2], flat["rb"][1::2] = b1, np.where((d == 0) | (d == 3), p2, 2 * L_PAC - 1 - p2)
    flat["re"] = flat["rb"] + 100
    return [flat[i:i + 1] for i in range(len(flat))]


def _finish_case(pkg, L, cands, o=None):  # noqa: N803
    o = sam_opt() if o is None else o
    vecs = _vectors_for(cands)
    want_w = np.array([d << 30 | int(x) for d, x in cands], dtype=np.uint32)
    w = pkg.pestat_candidates(o, L_PAC, vecs)
    assert (w == want_w).all()
    pes = pkg.pestat_from_candidates(o, want_w)
    assert bits(pes) == bits(whole(L, o, vecs, L_PAC))
    return pes


def test_finish_at_min_dir_cnt(pkg, L):  # noqa: F811
    rng = np.random.default_rng(1)
    nine = [(1, x) for x in rng.integers(300, 500, 9)]
    pes = _finish_case(pkg, L, nine + [(2, x) for x in rng.integers(300, 500, 10)])
    assert list(pes["failed"]) == [1, 1, 0, 1]  # 9: not enough pairs; 10: enough


def test_finish_with_all_candidates_equal(pkg, L):  # noqa: F811
    pes = _finish_case(pkg, L, [(1, 400)] * 50)
    assert pes["failed"][1] == 0 and pes["avg"][1] == 400.0 and pes["std"][1] == 0.0 and pes["low"][1] == pes["high"][1] == 400


def test_finish_at_min_dir_ratio(pkg, L):  # noqa: F811
    rng = np.random.default_rng(2)
    big = [(1, x) for x in rng.integers(300, 500, 400)]
    under = _finish_case(pkg, L, big + [(0, x) for x in rng.integers(200, 260, 19)])  # 19 < 0.05 * 400: dropped although it had enough pairs
    at = _finish_case(pkg, L, big + [(0, x) for x in rng.integers(200, 260, 20)])     # 20 == 0.05 * 400: kept
    assert under["failed"][0] == 1 and under["high"][0] > 0 and at["failed"][0] == 0


def test_finish_on_200000_candidates_with_long_equal_runs(pkg, L):  # noqa: F811
    rng = np.random.default_rng(3)
    x = np.clip(np.rint(rng.normal(400, 60, 200_000)), 1, 10_000).astype(np.int64)
    pes = _finish_case(pkg, L, [(1, v) for v in x])
    assert pes["failed"][1] == 0 and abs(pes["avg"][1] - 400) < 1 and abs(pes["std"][1] - 60) < 2
    assert np.bincount(x).max() > 1000  # long runs of equal values under the ordered sums


# ---------------------------------------------------------------- the core as a stand-alone program

def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-lm"], capture_output=True, text=True)
    return gcc, exe, cc


def _write_case(path, o, l_pac, vecs, lens, drop):
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiiq", 0x50455354, int(drop), int(o["a"]), len(vecs), int(l_pac)))
        f.write(o.tobytes())
        f.write(np.asarray(lens, dtype="<i4").tobytes())
        f.write(np.array([len(v) for v in vecs], dtype="<i4").tobytes())
        f.write(np.concatenate([np.zeros(0, dtype=kswlib.ALNREG)] + [np.asarray(v, dtype=kswlib.ALNREG) for v in vecs]).tobytes())


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    print(run.stdout.strip())
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    m = re.fullmatch(r"pairs (\d+) nonzero (\d+) removed (\d+) digest (\d+)\s*", run.stdout)
    assert m, run.stdout
    return tuple(int(x) for x in m.groups())


@pytest.fixture(scope="module")
def program_cases(pkg, tmp_path_factory):
    """(file, what the library gives for it) per case: the hand-made vectors and 100 000 random pairs, without and with drop-exact"""
    d = tmp_path_factory.mktemp("pestat_cases")
    o = sam_opt(max_ins=600)
    sets = {"handmade": (pr.handmade(o, L_PAC), None)}
    rv, rl = pr.random_vectors(np.random.default_rng(11), 100_000, L_PAC, 600, exact_share=0.15)
    sets["random"] = (rv, rl)
    # the hand-made vectors again with every third head region an exact match, so that the move runs on 1-, 2- and 40-region slices
    hv = [v.copy() for v in sets["handmade"][0]]
    for k, v in enumerate(hv):
        if len(v) and k % 3 == 0:
            v["truesc"][0] = 100
    out = []
    for name, (vecs, lens) in {**sets, "handmade_exact": (hv, None)}.items():
        lens = np.full(len(vecs), 100, dtype=np.int32) if lens is None else lens
        for drop in (0, 1):
            path = d / f"{name}_{drop}.bin"
            _write_case(path, o, L_PAC, vecs, lens, drop)
            kept, gone = pr.drop_exact(vecs, lens, int(o["a"])) if drop else (vecs, 0)
            w = pkg.pestat_candidates(o, L_PAC, kept)
            out.append((f"{name}_{drop}", path, (len(w), int((w != 0).sum()), gone, pr.digest(w))))
    return out


def test_core_program_matches_the_library(program_cases, tmp_path):
    _, exe, cc = _build(tmp_path, "ps_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    for name, path, want in program_cases:
        assert _run(exe, path) == want, name
    by = {n: w for n, _, w in program_cases}
    assert by["random_1"][2] > 10_000 and by["random_0"][1] > 20_000 and by["handmade_exact_1"][2] > 20
    assert by["random_1"][3] != by["random_0"][3]  # the move changes the words


def test_core_program_under_sanitizer_with_exact_blocks(program_cases, tmp_path):
    gcc, _, plain = _build(tmp_path, "ps_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "ps_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    for name, path, want in program_cases:
        assert _run(exe, path) == want, name
