"""The three paths of the exact introsort (host/sort_exact.h) on the host: quicksort, final insertion sort and the combsort
fallback that only an adversarial or already ordered input reaches.  tests/sortmodel.py restates the routine to PROVE which path an
input takes (coverage conditions and the range-stack bound below); what the routines must OUTPUT comes from the compiled
reference's mem_sort_and_dedup, mem_mark_primary_se and mem_chain_flt over the same inputs (tests/golden/sort_paths_golden.npz,
tools/make_sort_fixture.py).  The gcc build of the text is checked here -- bmh_sort_and_dedup, bmh_mark_primary_se,
bmh_chain_reads -- and once more as a stand-alone program (tests/sort_paths_main.c) under AddressSanitizer with a heap range stack of exactly
bmh_sort_stack_len(n) entries; the hipcc build in tests/test_sort_paths_gpu.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import kswlib
import reflib
import sortmodel as sm
from __graft_entry__ import load_package
from test_chain_cpu import run_chain_reads
from test_postproc_cpu import L, sam_opt  # noqa: F401  (L: the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK_ID0 = 12345  # tools/make_sort_fixture.py


@pytest.fixture(scope="module")
def fx():
    return sm.fixture()


# ---- a) coverage conditions ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traces():
    """name -> model trace of the sort the case is built for, over the case's own records under that sort's own comparator."""
    out = {}
    for n in sm.SIZES:
        for name, keys in sm.sequences(n).items():
            out[f"keys_{name}_{n}"] = sm.trace_keys(keys)
            out[f"chain_{name}_{n}"] = sm.trace_chain_sort(sm.chain_seeds(keys))
            if sm.first_built(name, n):
                out[f"first_{name}_{n}"] = sm.trace_first_sort(sm.regions_first(keys))
            if sm.second_built(name, n):
                out[f"second_{name}_{n}"] = sm.trace_second_sort_unthinned(sm.regions_second(keys))
        if n <= sm.MIXED_MAX:
            for fold in (2, 8):
                out[f"mixed_div{fold}_{n}"] = sm.trace_first_sort(sm.regions_mixed(sm.killer(n)[0], fold))
    return out


def test_the_model_sorts_and_replays():
    """The restatement is a sort, and the adversary's frozen values take the path of the adversarial run itself."""
    rng = np.random.default_rng(5)
    for n in list(range(0, 70)) + [257, 1000]:
        keys = [int(x) for x in rng.integers(0, max(1, n // 3 + 1), size=n)]
        sm.trace_keys(keys)  # asserts sortedness
    for n in sm.SIZES:
        keys, tr = sm.killer(n)
        assert sm.trace_keys(keys).key() == tr.key(), n


def test_shuffled_inputs_never_reach_combsort():
    """Why the fixture is needed: random orders stay inside the depth budget."""
    rng = np.random.default_rng(6)
    for n in (17, 40, 100, 300, 1000, 2000):
        for _ in range(5):
            assert sm.trace_keys([int(x) for x in rng.permutation(n)]).comb == []


def test_paths_covered(traces, fx):
    # every adversary sequence of n >= 40 calls combsort, under each of the three comparators the builders target
    for n in sm.SIZES:
        for kind in ("keys", "first", "second", "chain"):
            tr = traces[f"{kind}_killer_{n}"]
            if n >= 40:
                assert len(tr.comb) >= 1, f"{kind} killer n={n}: no combsort call; partitions {tr.partitions}"
            assert tr.key() == traces[f"keys_killer_{n}"].key(), f"{kind} killer n={n}: the builder does not keep the order"
    # for each n >= 64 at least one tie-folded variant does too, under each comparator
    for n in (x for x in sm.SIZES if x >= 64):
        for kind in ("first", "second", "chain"):
            if kind == "second" and n > sm.MIXED_MAX:
                continue  # (tied records of the second sort's vectors overlap across the whole vector: not built past MIXED_MAX)
            hit = {v: traces[f"{kind}_{v}_{n}"].comb for v in sm.TIE_FOLDED}
            assert any(hit.values()), f"{kind} n={n}: no tie-folded variant reaches combsort: {hit}"
        if n <= sm.MIXED_MAX:
            hit = {f: traces[f"mixed_div{f}_{n}"].comb for f in (2, 8)}
            assert any(hit.values()), f"mixed n={n}: {hit}"
    # the combsort ranges of the fixture's cases span 18..1900, and many gaps
    names = {name for name, _ in fx["regs"]} | {name for name, _ in fx["chains"]}
    assert names <= set(traces), names - set(traces)
    sizes = sorted({s for name in names for s in traces[name].comb})
    gaps = sorted({g for name in names for g in traces[name].comb_gaps})
    assert sizes and sizes[0] <= 18 and sizes[-1] >= 1900, f"combsort range sizes over the fixture: {sizes}"
    assert {11, 2, 3}.issubset(gaps) and 9 not in gaps and 10 not in gaps and len(gaps) >= 40, gaps
    # the other two paths
    assert all(traces[f"keys_{name}_2"].n2 for name in sm.sequences(2))
    for n in (3, 16, 17):
        assert traces[f"keys_killer_{n}"].insertion_only and traces[f"first_killer_{n}"].insertion_only, n
    assert not traces["keys_killer_33"].insertion_only and traces["keys_killer_33"].comb == []  # quicksort beyond the first partition, no combsort


def test_range_stack_bound(traces):
    """bmh_sort_stack_len(n) entries suffice -- over every generated sequence, further structured and random ones, and so do the
    device's fixed arrays (kDedupStk = 34 in csrc/chain2reg.hip, BMH_CC_STK = 40 in host/chain_core.h)."""
    worst = 0
    for name, tr in traces.items():
        assert tr.max_stack <= sm.stack_len(tr.n), (name, tr.max_stack, sm.stack_len(tr.n))
        worst = max(worst, tr.max_stack)
    rng = np.random.default_rng(7)
    for n in (18, 33, 64, 100, 257, 1000, 2000, 5000):
        for keys in ([int(x) for x in rng.permutation(n)], [int(x) for x in rng.integers(0, 4, size=n)],
                     [min(i, n - i) for i in range(n)], [(i * 37) % 101 for i in range(n)]):
            tr = sm.trace_keys(keys)
            assert tr.max_stack <= sm.stack_len(n), (n, tr.max_stack)
            worst = max(worst, tr.max_stack)
    assert 2 <= worst <= sm.stack_len(2 ** 31 - 1) <= 34 <= 40


# ---- c) the host routines against the fixture ---------------------------------------------------------------------------------

def _host_dedup(lib, v, level):
    a = v.copy()
    n = lib.bmh_sort_and_dedup(len(a), a.ctypes.data_as(C.c_void_p), C.c_float(level))
    return a[:n].copy()


def _host_mark(lib, o, a, ident):
    a = a.copy()
    lib.bmh_mark_primary_se(o.ctypes.data_as(C.c_void_p), len(a), a.ctypes.data_as(C.c_void_p), C.c_int64(ident))
    return a


def test_sort_and_dedup_matches_the_reference_fixture(L, fx):  # noqa: F811
    differ = 0
    for level in sm.LEVELS:
        for (name, v), want in zip(fx["regs"], fx["reg_want"][level]):
            got = _host_dedup(L, v, level)
            assert got.tobytes() == want.tobytes(), f"{name} at {level}: host keeps records {list(got['seedcov'][:40])}, reference {list(want['seedcov'][:40])}"
    # the fixture is about tie order: the levels below 1.0 and 1.0 itself keep DIFFERENT records of the tied groups
    for a, b in zip(fx["reg_want"][0.95], fx["reg_want"][1.0]):
        differ += a.tobytes() != b.tobytes()
    assert differ >= 30, differ


def test_mark_primary_matches_the_reference_fixture(L, fx):  # noqa: F811
    """bmh_mark_primary_se over what 0.95 leaves: the order and the fields it decides, named on failure, then the records whole.  Its
    sort (score descending, then hash) meets the survivors in score order, which klib's median of three turns into the worst case:
    the model, fed the hashes the routine itself assigned, reports combsort for every long vector of distinct scores."""
    o = sam_opt()
    comb = {}
    for ci, ((name, _), a) in enumerate(zip(fx["regs"], fx["reg_want"][0.95])):
        got = _host_mark(L, o, a, MARK_ID0 + 7 * ci)
        cols = np.stack([got[k].astype(np.int64) for k in sm.MARK_FIELDS], axis=1) if len(got) else np.zeros((0, len(sm.MARK_FIELDS)), np.int64)
        want = fx["reg_marked"][ci]
        bad = np.nonzero((cols != want).any(axis=1))[0]
        assert len(bad) == 0, (f"{name}: primary marking differs first at position {bad[0]}: {dict(zip(sm.MARK_FIELDS, cols[bad[0]]))}, "
                               f"reference {dict(zip(sm.MARK_FIELDS, want[bad[0]]))}")
        assert sm.crc(got) == fx["reg_marked_crc"][ci], f"{name}: order, secondary, sub and sub_n agree, another field does not"
        if name.startswith(("first_killer_", "second_killer_", "first_ascending_", "second_descending_")) and len(a) <= 300:
            comb[name] = sm.trace_mark_sort(a, got).comb
    for name, c in comb.items():
        n = int(name.rsplit("_", 1)[1])
        if n >= 40 and not name.startswith(("first_killer_div", "second_killer_div")):
            assert c and max(c) >= n - 25, f"{name}: the sort inside primary marking stays out of combsort: {c}"
    assert sorted({max(c) for c in comb.values() if c})[-1] >= 280, comb


def _chain_opts():
    return [sm.chain_opt(kw) for kw in sm.CHAIN_OPTS]


def test_chain_reads_matches_the_reference_fixture(fx):
    lib = load_package().lib()
    lib.bmh_chain_reads.restype = C.c_int
    for o, want in zip(_chain_opts(), fx["chain_want"]):
        reads, calls, intvs, _, sa_pos, sa_k = sm.chain_batch_tables([s for _, s in fx["chains"]], o)
        got = run_chain_reads(lib, o, sm.CHAIN_L_PAC, reads, calls, intvs, sa_k, sa_pos)
        for (name, _), g, w in zip(fx["chains"], got, want):
            assert all(len(c) == 1 for c in g), name
            g = np.concatenate(g) if g else np.zeros(0, kswlib.SEED)
            assert g.tobytes() == w.tobytes(), f"{name}: host keeps chains {list(g['rbeg'][:40] // sm._CH_STEP - 1)}, reference {list(w['rbeg'][:40] // sm._CH_STEP - 1)}"
    dropped = [sum(len(s) for _, s in fx["chains"]) - sum(len(w) for w in want) for want in fx["chain_want"]]
    assert dropped[0] == 0 and dropped[1] > 1000, dropped  # the default ratio shows the whole order; the moved one drops the light chains


@pytest.mark.ref
def test_host_routines_match_the_live_reference(L, fx):  # noqa: F811
    if not reflib.have_ref_bwa():
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_sort_fixture as mk
    R = reflib.lib()
    R.mem_sort_and_dedup.restype = C.c_int
    R.mem_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]
    R.mem_mark_primary_se.restype = None
    R.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    opt = R.mem_opt_init()
    o = sam_opt()
    for level in sm.LEVELS:
        for ci, (name, v) in enumerate(fx["regs"]):
            want = mk.ref_dedup(R, v, level)
            got = _host_dedup(L, v, level)
            assert got.tobytes() == want.tobytes(), (name, level)
            assert _host_mark(L, o, got, 99 + ci).tobytes() == mk.ref_mark(R, opt, want, 99 + ci).tobytes(), (name, level)
    for kw, want in zip(sm.CHAIN_OPTS, fx["chain_want"]):
        opt.contents.mask_level, opt.contents.chain_drop_ratio = kw["mask_level"], kw["chain_drop_ratio"]
        for (name, s), w in zip(fx["chains"], want):
            assert mk.ref_chain_flt(R, opt, s).tobytes() == w.tobytes(), name


# ---- d) the same text as a stand-alone program under AddressSanitizer ---------------------------------------------------------

def test_dedup_core_under_sanitizer_with_exact_stack(fx, tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    src = os.path.join(ROOT, "tests", "sort_paths_main.c")
    exe = tmp_path / "sort_paths_prog"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # the program itself must compile: an error in it or in the headers it includes is a failure, never a skip
    plain = subprocess.run([gcc, "-O1", "-g", "-Wall", src, "-o", str(tmp_path / "plain_prog")], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    # whether this machine can build and start a sanitized program at all is asked of an empty one
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    static = ["-static-libasan", "-static-libubsan"]  # the runtimes linked in where the static ones exist
    for extra in (static, []):
        pr = subprocess.run([gcc, *san, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if pr.returncode == 0:
            break
    if pr.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (pr.stderr.strip().splitlines() or ["?"])[-1])
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *san, *extra, src, "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    assert kswlib.ALNREG.itemsize == 64
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(fx["regs"])))
        for ci, (name, v) in enumerate(fx["regs"]):
            f.write(struct.pack("<ii", len(v), len(sm.LEVELS)))
            f.write(v.tobytes())
            for level in sm.LEVELS:
                ix = fx["reg_want"][level][ci]["seedcov"].astype("<i4")
                f.write(struct.pack("<fi", level, len(ix)))
                f.write(ix.tobytes())
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-4000:]}"
    assert run.stdout.strip() == f"{len(fx['regs']) * len(sm.LEVELS)} runs, 0 differ"
