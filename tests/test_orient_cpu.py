"""Pairing and mate rescue with all four orientations of mem_infer_dir open (FF, FR, RF, RR), on the CPU: every other fixture and
generator of the suite makes FR libraries, under which one orientation's window, one branch of mem_matesw and a pair table without
offsets are all the code ever meets.  tests/golden/orient_golden.npz (tools/make_orient_fixture.py, from the compiled reference;
generators in tests/orientgen.py) holds
 * pairing groups: region vectors placed in each orientation, the reference's mem_pestat table and its mem_pair per pair;
 * rescue groups: read pairs with the mate in each orientation, the reference's phase-1 regions and its own mate rescue.
Here: the fixture covers what it is for (asserted on the reference's results alone); bmh_pestat / bmh_pair / bmh_decide_batch
against it and, where oracle/_ref is built, live on further seeds; the oracle's orc_matesw_pair against the rescue groups; and the
two cores as stand-alone programs (tests/decide_core_main.c, tests/matesw_core_main.c), plainly and under AddressSanitizer, on a
four-orientation group each."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import decidegen as dg
import kswlib
import mswgen
import orientgen as og
import postgen
import test_decide_cpu as tdc
import test_matesw_core_cpu as tmc
from __graft_entry__ import load_package
from test_postproc_cpu import L, ours_pairs, sam_opt  # noqa: F401  (L: the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_KEYS = [f"p{si}_{mix}_" for si in (0, 2) for mix in og.MIXES]
RESCUE_KEYS = ["rbytev0_", "rbytev1_", "rwordv0_", "rwordv1_"]
ID0 = 2000  # pair p is decided under id (ID0 >> 1) + p = 1000 + p, the fixture's


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def winners(l_pac, vecs, pr):
    """per orientation of mem_infer_dir (from z): in how many pairs it is the winning pair's"""
    won = [0] * 4
    for k in np.nonzero(pr[:, 0] > 0)[0]:
        won[og.infer_dir(l_pac, int(vecs[2 * k][pr[k, 3]]["rb"]), int(vecs[2 * k + 1][pr[k, 4]]["rb"]))[0]] += 1
    return won


def grew(orient, regs, exp):
    n = [0] * 4
    for k in range(len(orient)):
        n[int(orient[k])] += len(exp[2 * k]) > len(regs[2 * k]) or len(exp[2 * k + 1]) > len(regs[2 * k + 1])
    return n


# ---------------------------------------------------------------- what the fixture covers, by the reference's results alone

def test_fixture_groups_are_all_there():
    g = og.golden()
    assert [str(k) for k in g["pair_groups"]] == PAIR_KEYS and [str(k) for k in g["rescue_groups"]] == RESCUE_KEYS
    assert all(len(v) == 800 for _, _, _, _, v, _, _, _ in og.pairing_groups())


@pytest.mark.parametrize("si", [0, 2])
def test_all_four_groups_cover_every_orientation(si):
    key, _, _, l_pac, vecs, _, pes, pr = og.pairing_group(f"p{si}_all4_")
    assert (pes["failed"] == 0).all(), pes
    windows = [(int(p["low"]), int(p["high"])) for p in pes]
    assert len(set(windows)) == 4 and all(lo <= hi for lo, hi in windows), windows
    won = winners(l_pac, vecs, pr)
    print(key, "windows", windows, "won", dict(zip(og.NAMES, won)), "n_sub > 0:", int((pr[:, 2] > 0).sum()))
    assert min(won) >= 20, won
    assert (pr[:, 2] > 0).sum() >= 50
    several = sum(len(og.pair_candidates(l_pac, pes, vecs[2 * k], vecs[2 * k + 1])) >= 2 for k in range(len(pr)))
    assert several >= 20, several


def test_the_other_mixes_open_what_they_are_named_for():
    for si in (0, 2):
        _, _, _, _, _, _, pes, _ = og.pairing_group(f"p{si}_fr_rf_")
        assert pes["failed"].tolist() == [1, 0, 0, 1]
        _, _, _, l_pac, vecs, _, pes, pr = og.pairing_group(f"p{si}_ff_rr_")
        assert pes["failed"][0] == 0 and pes["failed"][3] == 0
        won = winners(l_pac, vecs, pr)
        assert won[0] >= 20 and won[3] >= 20, won


@pytest.mark.parametrize("key", RESCUE_KEYS)
def test_rescue_groups_rescue_in_every_orientation(key):
    _, _, _, pes, _, _, _, regs, orient, exp, n_sw, _ = next(x for x in og.rescue_groups() if x[0] == key)
    assert (pes["failed"] == 0).all()
    n = grew(orient, regs, exp)
    print(key, "pairs whose vector grew", dict(zip(og.NAMES, n)), "ksw_align2 calls", sum(n_sw))
    assert min(n) >= 10, n


# ---------------------------------------------------------------- the host routines against the reference

def _same_table(pes, want):
    for f in ("low", "high", "failed", "avg", "std"):
        assert (pes[f] == want[f]).all(), (f, pes, want)


@pytest.mark.parametrize("key", PAIR_KEYS)
def test_pestat_and_pair_match_reference_fixture(L, key):  # noqa: F811
    _, si, _, l_pac, vecs, _, want_pes, want_pr = og.pairing_group(key)
    pes, pr = ours_pairs(L, sam_opt(**postgen.OPTION_SETS[si]), vecs, l_pac)
    _same_table(pes, want_pes)
    assert (pr == want_pr).all(), f"{key}: pairing differs at {np.nonzero((pr != want_pr).any(axis=1))[0][:5]}"


@pytest.mark.ref
@pytest.mark.parametrize("seed", [1, 2])
def test_pestat_and_pair_match_live_reference(L, seed):  # noqa: F811
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_orient_fixture as mk
    for si in (0, 2):
        for mi, mix in enumerate(og.MIXES.values()):
            vecs, _ = og.paired_vectors4(np.random.default_rng(5000 + 100 * seed + 10 * si + mi), 600, 3_000_000, mix)
            want_pes, want_pr = mk.ref_pairing(reflib.lib(), postgen.OPTION_SETS[si], vecs, 3_000_000)
            pes, pr = ours_pairs(L, sam_opt(**postgen.OPTION_SETS[si]), vecs, 3_000_000)
            _same_table(pes, want_pes)
            assert (pr == want_pr).all(), (seed, si, mi, np.nonzero((pr != want_pr).any(axis=1))[0][:5])
            assert (pr[:, 0] > 0).sum() > 200


@pytest.mark.parametrize("key", PAIR_KEYS)
def test_decide_batch_on_the_pairing_groups(pkg, L, key):  # noqa: F811
    _, si, _, l_pac, vecs, _, pes, pr = og.pairing_group(key)
    o = dg.pe_opt(si)
    out = pkg.decide_batch(o, l_pac, pes, ID0, vecs)
    n_paired, n_won = dg.check_pe_composition(L, o, l_pac, pes, ID0, vecs, out)
    pd = out["pd"]
    assert (pd["score"] == pr[:, 0]).all() and (pd["sub"] == pr[:, 1]).all() and (pd["n_sub"] == pr[:, 2]).all()
    pair_won = (pd["paired"] != 0) & ((pd["extra_flag"] & 2) != 0)
    # z indexes the vectors as mem_mark_primary_se leaves them (hits of one score may have changed places): the reference's rows over those
    marked = og.marked_pair_res(key)
    assert (marked[:, :3] == pr[:, :3]).all()
    assert (pd["z"][pair_won] == marked[pair_won, 3:5]).all()
    assert n_won == pair_won.sum() and n_won > 50 and n_paired >= n_won, (n_paired, n_won)


@pytest.mark.parametrize("key", RESCUE_KEYS)
def test_oracle_matesw_matches_rescue_fixture(key):
    _, p, o, pes, l_pac, pac, reads, regs, _, exp, n_sw, level = next(x for x in og.rescue_groups() if x[0] == key)
    got, ns = kswlib.orc_matesw_pairs(p, o, l_pac, pac, pes, reads, regs, mswgen.bmh_dedup_callback(level))
    assert ns == n_sw and sum(ns) > 1500
    for k, (a, b) in enumerate(zip(got, exp)):
        assert len(a) == len(b) and a.tobytes() == b.tobytes(), f"{key}: vector {k}: got {a}, want {b}"


@pytest.mark.ref
def test_tool_reproduces_the_fixture(tmp_path):
    import reflib
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    path = tmp_path / "again.npz"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_orient_fixture.py"), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    # (the archive's members carry the time they were written: the arrays are what the seeds pin)
    a, b = og.golden(), np.load(path)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------- the cores as stand-alone programs, plainly and under a sanitizer

def _san_extra(gcc, tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        pr = subprocess.run([gcc, *tdc.SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            return extra
    pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizer"])
def test_decide_core_program_on_a_four_orientation_group(pkg, tmp_path, san):
    cs = []
    for key in ("p0_all4_", "p2_all4_"):
        _, si, _, l_pac, vecs, _, pes, _ = og.pairing_group(key)
        cs.append((dg.pe_opt(si), pes, l_pac, ID0, vecs[:400]))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for o, pes, l_pac, id0, vecs in cs:
            assert o.nbytes == 96 and pes.nbytes == 128
            f.write(o.tobytes() + pes.tobytes() + struct.pack("<qqii", l_pac, id0, len(vecs), 0))
            for v in vecs:
                f.write(struct.pack("<i", len(v)) + np.ascontiguousarray(v, dtype=kswlib.ALNREG).tobytes())
    gcc, exe, cc = tdc._build(tmp_path, "decide_plain", [])
    assert cc.returncode == 0, cc.stderr  # the program itself must compile: never a skip
    if san:
        _, exe, cc = tdc._build(tmp_path, "decide_san", tdc.SAN + _san_extra(gcc, tmp_path))
        assert cc.returncode == 0, cc.stderr
    got, want = tdc._run(exe, path), [l.rstrip() for l in tdc._expected(pkg, cs)]
    assert got == want


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitizer"])
def test_matesw_core_program_on_a_four_orientation_group(tmp_path, san):
    path = tmp_path / "cases.bin"
    keys = ("rwordv0_",)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(keys)))
        for x in og.rescue_groups():
            if x[0] in keys:
                _, p, o, pes, l_pac, pac, reads, regs, _, exp, n_sw, level = x
                tmc._case(f, p, o, pes, level, 0, l_pac, pac, reads, regs, exp, n_sw)
    gcc, exe, cc = tmc._build(tmp_path, "msw_plain", [])
    assert cc.returncode == 0, cc.stderr
    if san:
        _, exe, cc = tmc._build(tmp_path, "msw_san", tmc.SAN + _san_extra(gcc, tmp_path))
        assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-4000:]}"
    rows = [tuple(int(v) for v in m) for m in tmc.LINE.findall(run.stdout)]
    assert len(rows) == len(keys) and all(r[-1] == 0 for r in rows), run.stdout
    assert all(r[1] == 400 and r[4] > 1500 for r in rows), rows  # every ksw_align2 call of the reference's loop
