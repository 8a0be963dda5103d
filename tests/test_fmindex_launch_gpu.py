"""Builds and launch shapes of the SMEM kernels that the library's own choices never reach on a small batch: the
five-waves-per-SIMD builds (BMH_SMEM_WAVES=5), partial waves and larger grids (BMH_SMEM_LANES), the conv kernel's
"wait until N lanes have a finished call" rule (BMH_SMEM_EMIT) at batch sizes around the rule's threshold and the wave
size, degenerate batches, and the host reorder path (BMH_SMEM_HOST_ORDER=1, in a child process).  Fixture index,
option sets `fixture` and `eager`, every read against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kswlib
from test_fmindex_cpu import _orc_calls, _same_calls, option_matrix_reads_and_oracle
from test_fmindex_gpu import KERNELS
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

SETS = ("fixture", "eager")
_cache = {}


def _golden():
    """the fixture index, loaded once for the module"""
    if "golden" not in _cache:
        _cache["golden"] = kswlib.golden_fmindex()
    return _cache["golden"]


def _run_and_compare(reads, want_of, label):
    """reads through bmh_smem_batch on a fresh context under both option sets; want_of(oname) = the oracle's answers"""
    cb, keep, raw, opt, _, per, sa_k, sa_pos = _golden()
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    for oname in SETS:
        got = ctx.smem_batch(kswlib.smem_option_set(oname), reads)
        assert len(got) == len(reads)
        for r, (g, w) in enumerate(zip(got, want_of(oname))):
            assert _same_calls(g, w), f"{label} {oname} read {r} (len {len(reads[r])})"
    ctx.close()


def _matrix_want(n=None):
    more, want = option_matrix_reads_and_oracle()
    return more[:n], lambda oname: want[oname, False][:n]


@pytest.mark.parametrize("kernel", KERNELS)
def test_five_wave_builds(kernel, monkeypatch):
    """smem_kernel<5> / smem_conv_kernel<5>: register allocations of their own, picked only above 262 144 reads"""
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    monkeypatch.setenv("BMH_SMEM_WAVES", "5")
    _run_and_compare(*_matrix_want(), f"waves 5 {kernel}")


@pytest.mark.parametrize("lanes", [8, 16, 32])
@pytest.mark.parametrize("kernel", KERNELS)
def test_fewer_reads_per_wave(kernel, lanes, monkeypatch):
    """BMH_SMEM_LANES: partial waves in the loop kernel (a stride of gridDim.x * lanes); the conv kernel ignores the lane
    count but gets the larger grid, so most of its waves draw nothing from the shared read counter"""
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    monkeypatch.setenv("BMH_SMEM_LANES", str(lanes))
    _run_and_compare(*_matrix_want(), f"lanes {lanes} {kernel}")


@pytest.mark.parametrize("emit", [1, 64])
def test_conv_emit_threshold(emit, monkeypatch):
    """emit the moment a lane has a finished call / only when the whole wave has one (or nobody is busy)"""
    monkeypatch.setenv("BMH_SMEM_KERNEL", "conv")
    monkeypatch.setenv("BMH_SMEM_EMIT", str(emit))
    _run_and_compare(*_matrix_want(), f"emit {emit}")


@pytest.mark.parametrize("emit", [None, 64])
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_sizes_around_the_wave_and_the_emit_threshold(kernel, emit, monkeypatch):
    """1 .. 129 reads: fewer lanes with work than the emit rule waits for, one wave exactly, one read more than a wave.
    "Fewer than emit_min lanes are waiting and nobody is busy" is what ends such a batch."""
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    if emit is not None:
        monkeypatch.setenv("BMH_SMEM_EMIT", str(emit))
    cb, keep, raw, opt, _, per, sa_k, sa_pos = _golden()
    more, want = option_matrix_reads_and_oracle()
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 129):
        for oname in SETS:
            lo = 200 + n  # a different window of the reads for every size
            got = ctx.smem_batch(kswlib.smem_option_set(oname), more[lo:lo + n])
            assert len(got) == n
            for r, (g, w) in enumerate(zip(got, want[oname, False][lo:lo + n])):
                assert _same_calls(g, w), f"{n} reads {kernel} emit {emit} {oname} read {r}"
    ctx.close()


def _degenerate_batches():
    if "degenerate" not in _cache:
        _cache["degenerate"] = _make_degenerate_batches()
    return _cache["degenerate"]


def _make_degenerate_batches():
    cb, keep, raw, opt, reads, per, sa_k, sa_pos = _golden()
    src = np.concatenate(reads)
    rng = np.random.default_rng(227)

    def cut(L):
        p = int(rng.integers(0, len(src) - L))
        return src[p:p + L].copy()

    n_ends = []
    for L in (2, 3, 20, 21, 80, 150):
        rd = cut(L)
        rd[0] = rd[-1] = 4
        n_ends.append(rd)
        rd = cut(L)
        rd[:min(3, L // 2)] = 4
        rd[-min(5, L // 2):] = 4
        n_ends.append(rd)
    alternating = []
    for L in (2, 3, 64, 65, 151):
        for first in (0, 1):
            rd = cut(L)
            rd[first::2] = 4
            alternating.append(rd)
    long_one = [cut(20) for _ in range(200)]
    long_one.insert(77, cut(5000))
    return {
        "empty_reads": [np.zeros(0, np.uint8) for _ in range(70)],
        "all_n_reads": [np.full(L, 4, np.uint8) for L in list(range(1, 67)) + [150, 300]],
        "one_base": [np.array([2], np.uint8)],
        "n_at_both_ends": n_ends,
        "base_n_alternating": alternating,
        "one_long_read": long_one,  # lcap comes from the longest read: 5 002 stack entries per lane for every lane
    }


@pytest.mark.parametrize("which", ["empty_reads", "all_n_reads", "one_base", "n_at_both_ends", "base_n_alternating", "one_long_read"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_degenerate_batches(kernel, which, monkeypatch):
    monkeypatch.setenv("BMH_SMEM_KERNEL", kernel)
    cb = _golden()[0]
    reads = _degenerate_batches()[which]
    want = {oname: [_orc_calls(cb, kswlib.smem_option_set(oname), rd) for rd in reads] for oname in SETS}
    if which in ("empty_reads", "all_n_reads"):
        assert all(len(c) == 0 and len(i) == 0 for c, i in want["fixture"])
    else:
        assert sum(len(c) for c, _ in want["fixture"]) >= 1
    _run_and_compare(reads, lambda oname: want[oname], f"{which} {kernel}")


def test_host_order_path_in_a_fresh_process():
    """BMH_SMEM_HOST_ORDER=1 (read once per process): the host reorder pass in the second half of smem_impl, for
    bmh_smem_batch and bmh_seed_batch.  One child, which compares with the oracle itself."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fmindex_host_order_child.py")
    env = dict(os.environ, BMH_SMEM_HOST_ORDER="1")
    for k in ("BMH_SMEM_KERNEL", "BMH_SMEM_WAVES", "BMH_SMEM_LANES", "BMH_SMEM_EMIT", "BMH_SMEM_INIT_CAP"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, child], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "mismatches: 0" in p.stdout
