"""Which bin of the global dispatcher a task goes to and its sort key there (host/glbbin_core.h, used by glb_sort_hist_kernel), said in
plain Python and without the C header; from it the per-bin counts bmh_last_global_bin_counts must report for a batch, the order
global_narrow_kernel meets the tasks of bins 6 and 7 in, and its seam waves."""
import numpy as np

import glbband_ref

EXACT_LOW, EXACT_ALL = 3, 7  # BMH_GLB_EXACT: bin 6 (bands 0..3) is on from 3, bin 7 (bands 4..7) at 7


def lane_bin(w, c32=1, exact=EXACT_ALL):
    """Bin of a task the lane kernels may take, from the band it runs on."""
    if exact >= EXACT_LOW and w <= 3:
        return 6
    if exact >= EXACT_ALL and w <= 7:
        return 7
    if c32 and w <= 15:
        return 5
    return 0 if w <= 31 else 3 if w <= 47 else 1 if w <= 63 else 2


def sort_key(b, tlen, w):
    rows = tlen >> 3
    if b in (2, 4):
        return 0
    if b in (6, 7):
        return (w & 3) << 9 | min(rows, 511)  # band-major
    return min(rows, 127) << 4 | (min(w, 63) >> (0 if b == 5 else 1 if b == 0 else 2) & 15)


def expected_bins(p, pool, tasks, narrow=True, c32=1, exact=EXACT_ALL, rows_cap=None, bands=None):
    """(bin, band the lane kernels run on) of every task of a batch whose queries all fit the wave kernel's LDS row (no bin 4).
    bands: glbband_ref.expected_bands of the batch, where the caller has them already."""
    if rows_cap is None:
        rows_cap = min(int(tasks["tlen"].max()), glbband_ref.ROWS_CAP) if len(tasks) else glbband_ref.ROWS_CAP
    if narrow and bands is None:
        bands = glbband_ref.expected_bands(p, pool, tasks, rows_cap)
    bins, ws = np.zeros(len(tasks), dtype=np.int64), np.zeros(len(tasks), dtype=np.int64)
    dom = glbband_ref.lane_domain_all(p, tasks, rows_cap)
    for k, x in enumerate(tasks):
        w = int(x["w"])
        b = 2
        if dom[k]:
            if narrow:
                w = int(bands[k])
            b = lane_bin(w, c32, exact)
        bins[k], ws[k] = b, w
    return bins, ws


def expected_counts(p, pool, tasks, **kw):
    return np.bincount(expected_bins(p, pool, tasks, **kw)[0], minlength=8).astype(np.uint32)


def narrow_waves(bins, ws, tlens, b):
    """The bands of every 64-task wave of bin b as global_narrow_kernel meets them: the bin's list sorted by key, read from its end.
    (The order inside one key is the sort's own; it does not change a wave's set of bands unless two keys of one band are split,
    which leaves the set as it is.)"""
    sel = np.nonzero(bins == b)[0]
    keys = np.array([sort_key(b, int(tlens[k]), int(ws[k])) for k in sel], dtype=np.int64)
    order = sel[np.argsort(keys, kind="stable")][::-1]
    return [sorted(set(int(ws[k]) for k in order[g:g + 64])) for g in range(0, len(order), 64)]


def seam_waves(bins, ws, tlens, b):
    return sum(len(x) > 1 for x in narrow_waves(bins, ws, tlens, b))
