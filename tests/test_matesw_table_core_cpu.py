"""host/matesw_table_core.h on the CPU: what mt_filter_kernel (csrc/matesw.hip) decides about every pair of a region table, and
bmh_matesw_device about the caller's vectors -- the candidate counts, the busy flag, the slice capacities, the reads' refusals -- as
tests/matesw_table_core_main.c runs it, against a plain Python restatement of bmh_matesw_device's host loop as it stood before the header
(pre-filter, n_hits, capacities and the per-read refusals), on seeded random tables with every clause in them.  Plainly, and under
AddressSanitizer with every vector in a heap block of its exact size."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kswlib

SRC = os.path.join(kswlib.ROOT, "tests", "matesw_table_core_main.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
L_PAC = 100_000
LOW, HIGH = 50, 600
RULE = np.dtype([("a", "<i4"), ("max_mat", "<i4"), ("score_limit", "<i4"), ("wide_sw", "<i4"), ("wraps", "<i4"), ("rsv", "<i4")])
HEAD = np.dtype([("n", "<i4", 2), ("l_seq", "<i8", 2)])
R_LEN, R_SCORE, R_GAPS = 1, 2, 3
# (name, (pen_unpaired, max_matesw), failed per orientation, (a, max_mat, wide_sw, wraps), pairs)
CASES = [("default_fr", (17, 100), (1, 0, 1, 1), (1, 1, 0, 0), 500), ("one_fr", (17, 1), (1, 0, 1, 1), (1, 1, 0, 0), 400),
         ("none_fr", (17, 0), (1, 0, 1, 1), (1, 1, 0, 0), 200), ("default_all", (17, 100), (0, 0, 0, 0), (2, 2, 0, 0), 300),
         ("all_failed", (17, 100), (1, 1, 1, 1), (1, 1, 0, 0), 200), ("wraps", (0, 3), (1, 0, 1, 1), (1, 1, 0, 1), 300),
         ("wide", (17, 100), (1, 0, 1, 1), (100, 100, 1, 0), 300), ("narrow", (17, 100), (1, 0, 1, 1), (100, 100, 0, 0), 300),
         ("negative_max", (17, -3), (1, 0, 1, 1), (1, 1, 0, 0), 100), ("no_pairs", (17, 100), (1, 0, 1, 1), (1, 1, 0, 0), 0)]
ODD_LENGTHS = (0, 0, 0, 65536, 65536, 65536, 65535, 1, 2, 3, 249, 250, 319, 320, 31999, 32000)


def _pes(failed):
    t = np.zeros(4, dtype=kswlib.PESTAT)
    t["low"], t["high"], t["avg"], t["std"] = LOW, HIGH, 300.0, 50.0
    t["failed"] = failed
    return t


def _vec(rng, rbs, pen):
    """regions at rbs: the first scores highest or not, the others on both sides of first - pen"""
    v = np.zeros(len(rbs), dtype=kswlib.ALNREG)
    if len(rbs):
        v["rb"] = rbs
        v["re"] = v["rb"] + 100
        v["qe"] = 100
        v["score"] = 100 - rng.integers(0, 2 * pen + 3, len(rbs))
        if rng.random() < 0.8:
            v["score"][0] = 100
        v["secondary"] = -1
    return v


def random_pairs(rng, n, pen):
    """per pair (v0, v1, l0, l1).  An anchor at b1 on the forward strand is covered under FR by a mate hit at 2 * L_PAC - 1 - (b1 + d),
    LOW <= d <= HIGH, and the other way round: such pairs need no rescue unless a candidate hit is left uncovered"""
    out = []
    for _ in range(n):
        kind = rng.integers(0, 8)
        k = int(rng.integers(1, 7))
        b1 = rng.integers(1000, L_PAC - 2000, k)
        d = rng.integers(LOW, HIGH + 1, k)
        b2 = 2 * L_PAC - 1 - (b1 + d)
        if kind == 0:
            rb0, rb1 = [], []
        elif kind == 1:
            rb0, rb1 = b1, []
        elif kind == 2:
            rb0, rb1 = [], b2
        elif kind in (3, 4):  # every hit covered
            rb0, rb1 = b1, b2
        elif kind == 5:  # some hits of end 0 uncovered
            rb0, rb1 = b1, b2[:int(rng.integers(0, k))]
        elif kind == 6:  # some hits of end 1 uncovered, out of the window by one base on either side
            rb0, rb1 = b1[:k // 2], np.concatenate([b2[:k // 2], 2 * L_PAC - 1 - (b1[k // 2:] + rng.choice([LOW - 1, HIGH + 1]))])
        else:  # same strand, both orders
            rb0, rb1 = b1, b1 + rng.integers(-HIGH, HIGH + 1, k)
        v0, v1 = _vec(rng, rb0, pen), _vec(rng, rb1, pen)
        if rng.random() < 0.5:
            v0, v1 = v1, v0
        ls = [int(rng.choice(ODD_LENGTHS)) if rng.random() < 0.25 else int(rng.integers(30, 400)) for _ in range(2)]
        out.append((v0, v1, ls[0], ls[1]))
    return out


# ---- the host loop of bmh_matesw_device as it stood before the header (csrc/matesw.hip), restated

def _infer_dir(b1, b2):
    r1, r2 = b1 >= L_PAC, b2 >= L_PAC
    p2 = b2 if r1 == r2 else 2 * L_PAC - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def _skips(pes, a_rb, ma):
    skip = [int(pes["failed"][r]) != 0 for r in range(4)]
    for b in ma["rb"]:
        r, dist = _infer_dir(int(a_rb), int(b))
        if pes["low"][r] <= dist <= pes["high"][r]:
            skip[r] = True
    return sum(skip)


def _n_hits(v, pen, max_matesw):
    nb, maxm = 0, max(max_matesw, 0)
    for j in range(len(v)):
        if not nb < maxm:
            break
        nb += int(v["score"][j] >= v["score"][0] - pen)
    return nb


def restate(pes, opt, rule, pairs):
    """per pair (nb0, nb1, busy, cap0, cap1, refuse0, refuse1)"""
    pen, max_matesw = opt
    a, max_mat, wide, wraps = rule
    out = []
    for v0, v1, l0, l1 in pairs:
        busy = False
        for v, ma in ((v0, v1), (v1, v0)):
            nb = 0
            for j in range(len(v)):
                if busy:
                    break
                if v["score"][j] < v["score"][0] - pen:
                    continue
                nb += 1
                if nb - 1 >= max_matesw:
                    break
                busy = _skips(pes, v["rb"][j], ma) != 4
            if busy:
                break
        nb = [_n_hits(v0, pen, max_matesw), _n_hits(v1, pen, max_matesw)]
        refuse = [0, 0]
        if busy:
            for i, l in enumerate((l0, l1)):
                xbyte = l * a < 250
                if l < 1 or l > 65535:
                    refuse[i] = R_LEN
                elif not (wide and not xbyte) and l * max_mat >= 32000:
                    refuse[i] = R_SCORE
                elif xbyte and wraps:
                    refuse[i] = R_GAPS
        out.append((nb[0], nb[1], int(busy), len(v0) + 4 * nb[1], len(v1) + 4 * nb[0], refuse[0], refuse[1]))
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per case (name, file, options, rule, pes, pairs, the restatement's answer)"""
    d = tmp_path_factory.mktemp("matesw_table_cases")
    out = []
    for k, (name, opt, failed, rule, n) in enumerate(CASES):
        pes = _pes(failed)
        pairs = random_pairs(np.random.default_rng(5200 + k), n, max(opt[0], 4))
        o = np.zeros((), dtype=kswlib.MATESW_OPT)
        o["pen_unpaired"], o["max_matesw"], o["min_seed_len"] = opt[0], opt[1], 19
        r = np.zeros((), dtype=RULE)
        r["a"], r["max_mat"], r["score_limit"], r["wide_sw"], r["wraps"] = rule[0], rule[1], 32000, rule[2], rule[3]
        head = np.zeros(n, dtype=HEAD)
        for p, (v0, v1, l0, l1) in enumerate(pairs):
            head[p]["n"], head[p]["l_seq"] = (len(v0), len(v1)), (l0, l1)
        path = d / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(np.array([0x4d545442, n], dtype="<i4").tobytes())
            f.write(np.array([L_PAC], dtype="<i8").tobytes())
            f.write(pes.tobytes() + o.tobytes() + r.tobytes() + head.tobytes())
            for v0, v1, _, _ in pairs:
                f.write(v0.tobytes() + v1.tobytes())
        out.append((name, path, opt, rule, pes, pairs, restate(pes, opt, rule, pairs)))
    return out


def _build(tmp_path, name, flags):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    exe = tmp_path / name
    cc = subprocess.run([gcc, "-O1", "-g", "-Wall", *flags, SRC, "-o", str(exe), "-lm"], capture_output=True, text=True)
    return gcc, exe, cc


def _check(exe, cases):
    for name, path, _, _, _, pairs, want in cases:
        run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert run.returncode == 0, f"{name}: exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
        got = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
        assert len(got) == len(pairs), name
        for p, (g, w) in enumerate(zip(got, want)):
            assert g == (p,) + w, f"{name}: pair {p}: got {g[1:]}, want {w} (nb0 nb1 busy cap0 cap1 refuse0 refuse1)"


def test_the_inputs_hold_every_clause(cases):
    by = {name: (opt, pairs, want) for name, _, opt, _, _, pairs, want in cases}
    _, pairs, want = by["default_fr"]
    busy = np.array([w[2] for w in want], dtype=bool)
    assert 100 < busy.sum() < len(pairs) - 100
    # empty vectors on either end, in busy and idle pairs
    assert sum(len(v0) == 0 and len(v1) > 0 for v0, v1, _, _ in pairs) > 20 and sum(len(v1) == 0 and len(v0) > 0 for v0, v1, _, _ in pairs) > 20
    assert sum(len(v0) == 0 and len(v1) == 0 for v0, v1, _, _ in pairs) > 20
    # scores on both sides of a[0].score - pen_unpaired, at it, and vectors whose first region is not their best
    flat = [(v["score"][1:] - (v["score"][0] - 17)) for v0, v1, _, _ in pairs for v in (v0, v1) if len(v) > 1]
    diff = np.concatenate(flat)
    assert (diff < 0).sum() > 100 and (diff > 0).sum() > 100 and (diff == 0).sum() > 10
    assert sum(len(v) > 1 and v["score"][0] < v["score"].max() for v0, v1, _, _ in pairs for v in (v0, v1)) > 20
    # counts that max_matesw cuts and counts that it does not
    assert max(max(w[0], w[1]) for w in want) >= 5 and {max(w[0], w[1]) for w in by["one_fr"][2]} == {0, 1}
    assert all(w[0] == 0 and w[1] == 0 and w[2] == 0 for w in by["none_fr"][2]) and all(w[2] == 0 for w in by["negative_max"][2])
    assert by["none_fr"][0][1] == 0 and by["one_fr"][0][1] == 1 and by["default_fr"][0][1] == 100
    assert sum(w[2] for w in by["one_fr"][2]) > 50
    # reads of 0 and 65536 bases in active and in inactive pairs; only the former are refused
    for odd in (0, 65536):
        hit = [(w[2], w[5 + i]) for (_, _, *ls), w in zip(pairs, want) for i in range(2) if ls[i] == odd]
        assert (1, R_LEN) in hit and (0, 0) in hit and (1, 0) not in hit and (0, R_LEN) not in hit, (odd, hit)
    assert any(w[2] and ls[i] == 65535 and w[5 + i] == 0 for (_, _, *ls), w in zip(by["wide"][1], by["wide"][2]) for i in range(2))
    # all four orientations failed: nobody is busy, whatever the vectors
    assert all(w[2] == 0 and w[5] == 0 and w[6] == 0 for w in by["all_failed"][2]) and max(w[0] for w in by["all_failed"][2]) >= 5
    # all four open: same-strand pairs count too
    assert sum(w[2] for w in by["default_all"][2]) > sum(w[2] for w in want) * 300 // 500
    # the other two refusals, and the wide switch taking word-mode reads only
    assert sum(R_GAPS in w[5:] for w in by["wraps"][2]) > 50
    assert sum(R_SCORE in w[5:] for w in by["narrow"][2]) > 50
    wide = [(ls[i], w[5 + i]) for (_, _, *ls), w in zip(by["wide"][1], by["wide"][2]) for i in range(2) if w[2]]
    assert any(320 <= l <= 65535 and r == 0 for l, r in wide) and all(r != R_SCORE for l, r in wide if l >= 3)  # (2 x 100 < 250: byte mode)
    assert any(r == R_SCORE for l, r in [(ls[i], w[5 + i]) for (_, _, *ls), w in zip(by["default_fr"][1], want) for i in range(2)] if l >= 32000)
    assert by["no_pairs"][2] == []


def test_core_program_matches_the_restatement(cases, tmp_path):
    _, exe, cc = _build(tmp_path, "mt_plain", ["-O2"])
    assert cc.returncode == 0, cc.stderr
    assert cc.stderr.strip() == "", cc.stderr  # -Wall clean
    _check(exe, cases)


def test_core_program_under_sanitizer_with_exact_blocks(cases, tmp_path):
    gcc, _, plain = _build(tmp_path, "mt_plain", [])
    assert plain.returncode == 0, plain.stderr  # the program itself must compile: never a skip
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([gcc, *SAN, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime: an empty program does not build with -fsanitize=address,undefined: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    _, exe, cc = _build(tmp_path, "mt_san", SAN + extra)
    assert cc.returncode == 0, cc.stderr
    _check(exe, cases)


def test_both_drivers_are_built_on_the_header():
    """bmh_matesw_device's host loop and mt_filter_kernel hold no rule of their own: host and device cannot drift apart"""
    msw = open(os.path.join(kswlib.ROOT, "bwa-mem-quickassist_amd", "csrc", "matesw.hip")).read()
    assert '#include "../host/matesw_table_core.h"' in msw
    host = msw[msw.index('extern "C" int bmh_matesw_device('):msw.index("// ---- the table form")]
    assert "bmh_mt_busy(" in host and "bmh_mt_nb(" in host and "bmh_mt_cap(" in host and "bmh_mt_refuse(" in host and "bmh_msw_skip(" not in host
    kern = msw[msw.index("void mt_filter_kernel("):msw.index("mt_block_excl_scan(MtSum v")]
    assert "bmh_mt_pair(" in kern and "pen_unpaired" not in kern and "score" not in kern
