"""Reads to SAM text through the device calls on one context (tests/pipechain.py), against the compiled reference's own output for the
same chunk (tests/golden/pipeline_golden.npz, tools/make_pipeline_fixture.py): bmh_seed_chain_regs_batch with the de-duplication and
the insert-size words behind it hands its regions to bmh_matesw_device, which hands its to bmh_phase2_text_device -- real seedcov,
truesc and w values, equal-score ties, regions in repeats, empty vectors next to full ones -- and the text is the reference's byte for byte, as is the
text of the shim's default route composed from the host-fed calls.  Between the two routes every hand-off is the same record for record,
so a difference names the stage that owns it before any text is compared.  Paired-end and single-end under mem_opt_init's options and
under -A 2 -B 5 -w 12 -r 1.2; in three slices; twice on a context with another batch between; host and device routes in turn on one
context; and chunks of two pairs, which have no reference text and are compared route against route."""
import numpy as np
import pytest

import pipechain as pc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def both(pkg):
    """per run (device_chain's hand-offs, host_chain's), each on a context of its own, computed once"""
    done = {}

    def get(name):
        if name not in done:
            r, out = pc.run(name), []
            for chain in (pc.device_chain, pc.host_chain):
                c = pc.new_context(pkg)
                try:
                    out.append(chain(c, r))
                finally:
                    c.close()
            done[name] = tuple(out)
        return done[name]
    return get


def _n_ops(line):
    cigar = line.split(b"\t")[5]
    return sum(ch in b"MIDNSHP=X" for ch in cigar) if cigar != b"*" else 0


def _long_cigar_lines(r):
    return sum(_n_ops(ln) > 24 for ln in r.sam.splitlines())


@pytest.mark.parametrize("name", pc.RUNS)
def test_hand_off_parity(both, name):
    """regs1, the insert-size words and table (bit patterns) and regs2 are the same between the two routes, in order, every field"""
    dev, host = both(name)
    r = pc.run(name)
    pc.assert_same_hand_offs(dev, host, name)
    # the regions are phase 1's own: equal-score ties of the repeat reads, empty vectors next to vectors of five (as the reference's
    # mem_align1_core leaves them for these reads: 15 to 27 ties, 10 to 42 empty vectors, 5 or 6 regions at the most)
    flat = np.concatenate(dev.regs1)
    assert sum(len(a) == 0 for a in dev.regs1) >= 10 and max(len(a) for a in dev.regs1) >= 5, name
    assert sum(len(a) > 1 and a[0]["score"] == a[1]["score"] for a in dev.regs1) >= 15, name
    assert len(np.unique(flat["seedcov"])) > 20, name
    assert not (flat["rb"] < 0).any() and not (flat["re"] < 0).any()  # (host/sam_post.c's documented deviation is not met here)
    if not r.pe:
        assert dev.pes is None and pc.first_region_difference(dev.regs2, dev.regs1) is None


@pytest.mark.parametrize("name", pc.RUNS)
def test_reference_parity(both, name):
    """both routes give the reference's SAM body byte for byte, split at its read boundaries; the hand-offs first, so that a
    difference is reported at the stage that makes it"""
    dev, host = both(name)
    r = pc.run(name)
    pc.assert_same_hand_offs(dev, host, name)
    pc.assert_text(dev, r, name + ", device route")
    pc.assert_text(host, r, name + ", host route")


def _assert_device_stats(dev, host, r, what):
    n_in, n_kept = dev.stats["dedup"]
    assert (n_in, n_kept) == (sum(map(len, host.raw)), sum(map(len, host.regs1))) and n_kept > 0, (what, n_in, n_kept)
    if r.name.endswith("0"):  # (under -w 12 the reads across the tandem duplications leave no redundant region)
        assert n_in > n_kept, (what, n_in, n_kept)
    lo = 0
    for st in dev.stats["slices"]:
        hi = lo + st["n_units"] * (2 if r.pe else 1)
        text = dev.text[int(dev.text_off[lo]):int(dev.text_off[hi])]
        got = (st["fallbacks"], st["sessions"], st["units"], st["reads"], st["lines"], st["text_bytes"])
        assert got == (0, 1, st["n_units"], hi - lo, text.count(b"\n"), len(text)), (what, st)
        mapped = sum(not int(ln.split(b"\t")[1]) & 4 for ln in text.splitlines())
        assert st["wanted"] == mapped, (what, st, mapped)
        long_lines = sum(_n_ops(ln) > 24 for ln in text.splitlines())
        assert st["redone"] >= long_lines, (what, st, long_lines)
        if st["redone"]:  # finished by the long round on the device, none redone with host copies
            assert st["reg2cigar"] == (st["redone"], st["redone"], 0), f"{what}: the long round (regions, finished on the device, redone on the host): {st['reg2cigar']}"
            assert st["region_long"][0] == st["redone"] and st["region_long"][1] > 24 * long_lines, (what, st["region_long"], st["redone"])
        lo = hi
    assert lo == len(r.reads)
    assert sum(st["redone"] for st in dev.stats["slices"]) >= _long_cigar_lines(r) >= 1, what
    if r.pe:
        assert len(dev.n_sw) == len(r.reads) // 2 and sum(k > 0 for k in dev.n_sw) >= 10, (what, dev.n_sw)
        assert int((dev.cand != 0).sum()) >= 100, what
        grew = sum(len(b) > len(a) for a, b in zip(dev.regs1, dev.regs2))
        assert grew >= 10, (what, grew)  # rescue placed mates


@pytest.mark.parametrize("name", pc.RUNS)
def test_the_stages_ran_on_the_device(both, name):
    dev, host = both(name)
    _assert_device_stats(dev, host, pc.run(name), name)


@pytest.mark.parametrize("name", pc.RUNS)
def test_three_slices(pkg, both, name):
    """rescue and phase 2 in three slices of whole pairs (reads), id0 the slice's first read: the same text"""
    dev, host = both(name)
    r = pc.run(name)
    bounds = pc.slice_bounds(r, 3)
    assert all(lo % 64 and lo < hi for lo, hi in bounds[1:]) and bounds[-1][1] == len(r.reads)
    c = pc.new_context(pkg)
    try:
        cut = pc.device_chain(c, r, slices=3)
    finally:
        c.close()
    assert len(cut.stats["slices"]) == 3
    pc.assert_same_hand_offs(cut, host, name + ", three slices")
    assert cut.text == dev.text and np.array_equal(cut.text_off, dev.text_off)
    pc.assert_text(cut, r, name + ", three slices")
    _assert_device_stats(cut, host, r, name + ", three slices")


def test_one_context_through_everything_twice_with_another_batch_between(pkg, both):
    """a stale workspace, bin-size hint or switch of any stage shows as a text that is no longer the reference's"""
    r, other = pc.run("pe0"), pc.run("se1")
    c = pc.new_context(pkg)
    try:
        for what, x in (("first", r), ("again", r), ("the other option set, single-end", other), ("after it", r)):
            got = pc.device_chain(c, x)
            pc.assert_same_hand_offs(got, both(x.name)[1], what)
            pc.assert_text(got, x, what)
            _assert_device_stats(got, both(x.name)[1], x, what)
    finally:
        c.close()


def test_host_after_device_and_device_after_host_on_one_context(pkg, both):
    r = pc.run("pe0")
    c = pc.new_context(pkg)
    try:
        for what, chain in (("host", pc.host_chain), ("device after host", pc.device_chain), ("host after device", pc.host_chain)):
            got = chain(c, r)
            pc.assert_same_hand_offs(got, both("pe0")[1], what)
            pc.assert_text(got, r, what)
    finally:
        c.close()


def test_a_small_chunk(pkg):
    """the first two pairs alone, then the first pair beside a pair of one-base reads (bmh_matesw_batch takes no read without a base):
    with so few pairs every orientation fails, as in the reference's mem_pestat.  There is no reference text for these chunks: the two
    routes are compared with each other, hand-off by hand-off and then the text."""
    r = pc.run("pe0")
    one = [np.array([2], dtype=np.uint8), np.array([1], dtype=np.uint8)]
    chunks = {"two pairs": pc.sub_run(r, r.reads[:4], r.names[:4], r.quals[:4]),
              "a pair and a pair of one-base reads": pc.sub_run(r, r.reads[:2] + one, r.names[:2] + [b"tiny", b"tiny"], r.quals[:2] + [b"I", None])}
    c = pc.new_context(pkg)
    try:
        for what, x in chunks.items():
            dev, host = pc.device_chain(c, x), pc.host_chain(c, x)
            pc.assert_same_hand_offs(dev, host, what)
            assert [int(f) for f in dev.pes["failed"]] == [1, 1, 1, 1], (what, dev.pes)
            assert dev.text == host.text and np.array_equal(dev.text_off, host.text_off), (what, dev.text, host.text)
            assert dev.text.count(b"\n") >= 4 and sum(len(a) for a in dev.regs1[:2]) >= 2
    finally:
        c.close()

