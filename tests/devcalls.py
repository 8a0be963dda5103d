"""Device-resident calls for the GPU tests: numpy records up to torch buffers, result buffers filled with a poison byte
before the call (a slot the kernels never wrote can then not pass by accident), results back as numpy records.  The
callers decide how to wait: ctx.sync() on the context's own stream, or the caller's stream."""
import numpy as np

import kswlib

POISON = 0xA5
INT32_MIN = -2 ** 31
EXT_FAIL = (INT32_MIN, 0, 0, 0, 0, 0)           # what the extension kernels write for a task outside the range
SEED_FAIL = (0, 0, 0, 0, INT32_MIN, INT32_MIN, 0, 0)  # ... and the fused per-seed record of a seed outside it


def _torch():
    import torch
    return torch


def dev():
    return _torch().device("cuda:0")


def up(a):
    """A numpy array (any record dtype) as a uint8 tensor on the device."""
    a = np.ascontiguousarray(a)
    b = a.view(np.uint8).reshape(-1) if a.size else np.zeros(16, np.uint8)
    return _torch().from_numpy(b.copy()).to(dev())


def poisoned(nbytes):
    return _torch().full((max(int(nbytes), 16),), POISON, dtype=_torch().uint8, device=dev())


def down(t, dtype, n):
    return t.cpu().numpy()[: n * np.dtype(dtype).itemsize].view(dtype).copy()


class Ext:
    """One extension batch staged on the device: ext = Ext(pool, tasks, order); ext.run(ctx); wait; ext.result()."""

    def __init__(self, pool, tasks, order=None):
        self.n = len(tasks)
        self.pool, self.tasks = up(pool), up(tasks)
        self.order = up(np.asarray(order, dtype=np.uint32)) if order is not None else None
        self.res = poisoned(self.n * kswlib.EXT_RES.itemsize)
        _torch().cuda.synchronize()

    def run(self, ctx):
        ctx.extend_batch_device(self.pool.data_ptr(), self.tasks.data_ptr(), self.n, self.res.data_ptr(),
                                self.order.data_ptr() if self.order is not None else 0)

    def result(self):
        return down(self.res, kswlib.EXT_RES, self.n)


class Seed:
    def __init__(self, pool, tasks):
        self.n = len(tasks)
        self.pool, self.tasks = up(pool), up(tasks)
        self.res = poisoned(self.n * kswlib.SEED_RES.itemsize)
        _torch().cuda.synchronize()

    def run(self, ctx):
        ctx.seedext_batch_device(self.pool.data_ptr(), self.tasks.data_ptr(), self.n, self.res.data_ptr())

    def result(self):
        return down(self.res, kswlib.SEED_RES, self.n)


class Glb:
    def __init__(self, pool, tasks, words, order=None):
        self.n, self.words = len(tasks), max(int(words), 1)
        self.pool, self.tasks = up(pool), up(tasks)
        self.order = up(np.asarray(order, dtype=np.uint32)) if order is not None else None
        self.res = poisoned(self.n * kswlib.GLB_RES.itemsize)
        self.cig = poisoned(self.words * 4)
        _torch().cuda.synchronize()

    def run(self, ctx):
        ctx.global_batch_device(self.pool.data_ptr(), self.tasks.data_ptr(), self.n, self.res.data_ptr(), self.cig.data_ptr(),
                                self.order.data_ptr() if self.order is not None else 0)

    def result(self):
        return down(self.res, kswlib.GLB_RES, self.n), down(self.cig, np.uint32, self.words)


class Sw:
    def __init__(self, pool, tasks):
        self.n = len(tasks)
        self.pool, self.tasks = up(pool), up(tasks)
        self.res = poisoned(self.n * kswlib.SW_RES.itemsize)
        _torch().cuda.synchronize()

    def run(self, ctx):
        ctx.sw_batch_device(self.pool.data_ptr(), self.tasks.data_ptr(), self.n, self.res.data_ptr())

    def result(self):
        return down(self.res, kswlib.SW_RES, self.n)


# ---- comparisons: the index of the first difference in the message ---------------------------------------------------

def assert_ext(got, want, tasks, what=""):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}{len(bad)} of {len(got)} extension results differ; first {bad[0]}: task={tasks[bad[0]]} gpu={got[bad[0]]} want={want[bad[0]]}"


def assert_seed(got, want, tasks, what=""):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}{len(bad)} of {len(got)} seed records differ; first {bad[0]}: task={tasks[bad[0]]} gpu={got[bad[0]]} want={want[bad[0]]}"


def assert_glb(res, cig, want, wcig, tasks, what=""):
    bad = np.nonzero(res != want)[0]
    assert len(bad) == 0, f"{what}{len(bad)} of {len(res)} global results differ; first {bad[0]}: task={tasks[bad[0]]} gpu={res[bad[0]]} want={want[bad[0]]}"
    # every task's words [cigar_off, cigar_off + n_cigar) where it wanted a CIGAR and it fitted, gathered in one go
    n, cap = res["n_cigar"].astype(np.int64), tasks["cigar_cap"].astype(np.int64)
    n = np.where((cap > 0) & (n > 0) & (n <= cap), n, 0)
    first = np.cumsum(n) - n
    idx = np.repeat(tasks["cigar_off"].astype(np.int64) - first, n) + np.arange(int(n.sum()))
    diff = np.nonzero(cig[idx] != wcig[idx])[0]
    assert len(diff) == 0, f"{what}task {np.searchsorted(first, diff[0], side='right') - 1}: CIGAR words differ"


def assert_sw(got, want, tasks, what=""):
    for f in kswlib.SW_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}{len(bad)} Smith-Waterman results differ in {f}; first {bad[0]}: task={tasks[bad[0]]} gpu={got[bad[0]]} want={want[bad[0]]}"
