"""The FM-index kernels on tiny and degenerate indices (tests/tinyindex.py): fewer rows than a block, than an SA sample
interval, exactly one and two blocks, partial last blocks and words, absent bases (L2[c+1] == L2[c], empty start
intervals), primary == 1, == seq_len and in the last block -- every row through bmh_sa_batch against the plain suffix
sort, and bmh_smem_batch / bmh_seed_batch under every seeding option set against the oracle, which
tests/test_tiny_index_cpu.py pins to the reference on these very indices."""
import numpy as np
import pytest

import kswlib
import tinyindex as ti
from test_fmindex_cpu import _intv_len, _orc_calls, _same_calls
from test_fmindex_gpu import KERNELS
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

NAMES = list(ti.SHAPES)
CONFIGS = [(oname, emit) for oname in kswlib.SMEM_OPTION_SETS for emit in (False, True)]
NONE = np.uint64(ti.U64_MAX)
_want = {}


def _oracle(name):
    """reads of a shape and the oracle's answer under every (option set, emit), computed once and shared by both kernels"""
    if name not in _want:
        raw, _ = ti.shape(name)
        cb = kswlib.make_cbwt(*raw, keep := [])
        reads = ti.reads_for(name)
        _want[name] = reads, {cfg: [_orc_calls(cb, kswlib.smem_option_set(*cfg), rd) for rd in reads] for cfg in CONFIGS}
    return _want[name]


@pytest.mark.parametrize("name", NAMES)
def test_sa_batch_matches_plain_sort_on_every_row(name):
    raw, sa = ti.shape(name)
    ctx = _ctx_with({})  # a fresh context per shape: the device's index cache is keyed on the shape, so this rebinds too
    ctx.set_bwt(*raw)
    rows = np.arange(raw[2] + 1, dtype=np.uint64)
    assert (ctx.sa_batch(rows) == ti.sa_rows(sa)).all()
    assert (ctx.sa_batch(rows[::-1].copy()) == ti.sa_rows(sa)[::-1]).all()
    ctx.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_smem_matches_oracle_under_every_option_set(kernel, name, monkeypatch):
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    raw, _ = ti.shape(name)
    reads, want = _oracle(name)
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    for cfg in CONFIGS:
        got = ctx.smem_batch(kswlib.smem_option_set(*cfg), reads)
        for r, (g, w) in enumerate(zip(got, want[cfg])):
            assert _same_calls(g, w), f"{name} {cfg} read {r}: {reads[r].tolist()}"
    ctx.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_seed_batch_positions_are_the_suffix_array_rows(kernel, name, monkeypatch):
    """Every interval bmh_seed_batch looks up (length >= min_seed_len, x[2] <= max_occ) carries sa[x0 .. x0+x2) of the plain
    sort, every other one UINT64_MAX, and the position array holds nothing else."""
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    raw, sa = ti.shape(name)
    rows = ti.sa_rows(sa)
    reads, want = _oracle(name)
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    n_looked = 0
    for oname in ("fixture", "eager"):
        o = kswlib.smem_option_set(oname)
        for max_occ in (1, 3, 10000):
            got, offs, pos = ctx.seed_batch(o, max_occ, reads)
            n_pos = 0
            for r, ((gc, gi), so, w) in enumerate(zip(got, offs, want[oname, False])):
                assert _same_calls((gc, gi), w), f"{name} {oname} read {r}"
                look = (_intv_len(gi) >= int(o["min_seed_len"])) & (gi["x2"] <= np.uint64(max_occ))
                assert ((so != NONE) == look).all(), f"{name} {oname} max_occ {max_occ} read {r}"
                for k in np.nonzero(look)[0]:
                    x0, x2, b = int(gi["x0"][k]), int(gi["x2"][k]), int(so[k])
                    assert b + x2 <= len(pos) and (pos[b:b + x2] == rows[x0:x0 + x2]).all(), f"{name} {oname} read {r} interval {k}"
                    n_pos += x2
                    n_looked += 1
            assert n_pos == len(pos)
    assert n_looked > 50
    ctx.close()
