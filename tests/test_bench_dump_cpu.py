"""bench.py --dump-outputs on host tensors: the sampled records are the ones at the dumped indices, every field exact in float64,
the CIGAR words are the last chunk's for its sampled tasks, the whole dump stays inside its budget and repeats bit for bit."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench
import kswlib
from __graft_entry__ import load_package

pkg = load_package()


def _records(rng, dtype, n):
    return rng.integers(-2**31, 2**31, size=(n, dtype.itemsize // 4), dtype=np.int64).astype(np.int32)


def _case(seed=3):
    rng = np.random.default_rng(seed)
    chunks, host_recs = [], {"sres": [], "gres": []}
    gtasks_last = None
    for n, ng in ((700, 500), (900, 650)):
        s, g = _records(rng, pkg.SEED_RES, n), _records(rng, pkg.GLB_RES, ng)
        g[:, 1] = rng.integers(1, 6, size=ng)  # n_cigar
        host_recs["sres"].append(s)
        host_recs["gres"].append(g)
        gt = np.zeros(ng, pkg.GLB_TASK)
        gt["cigar_off"] = np.concatenate([[0], np.cumsum(g[:, 1])[:-1]])
        gtasks_last = gt
        chunks.append({"sres": torch.from_numpy(s.view(np.uint8).reshape(-1).copy()), "n": n,
                       "gres": torch.from_numpy(g.view(np.uint8).reshape(-1).copy()), "ng": ng})
    sw = _records(rng, pkg.SW_RES, 300)
    swb = [{"swres": torch.from_numpy(sw.view(np.uint8).reshape(-1).copy()), "ns": 300}]
    cig = rng.integers(0, 2**32, size=int(host_recs["gres"][-1][:, 1].sum()) + 8, dtype=np.uint64).astype(np.uint32)
    d_cig = torch.from_numpy(cig.view(np.int32).copy())
    return chunks, swb, d_cig, gtasks_last, host_recs, sw, cig


def test_dump_outputs_match_the_records(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", {"seedext": 1000, "global": 800, "rescue": 10_000})
    chunks, swb, d_cig, gtl, recs, sw, cig = _case()
    d = bench.dump_outputs(str(tmp_path / "a"), torch, pkg, kswlib, chunks, swb, d_cig, gtl)
    ld = lambda n: np.load(tmp_path / "a" / (n + ".npy"))
    assert d["bytes"] <= bench.DUMP_BYTES and all(ld(f[:-4]).dtype == np.float64 for f in d["files"])
    assert d["bytes"] == sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in d["files"])  # .npy header: 128 bytes
    for stage, full, names in (("seedext", np.concatenate(recs["sres"]), pkg.SEED_RES.names),
                               ("global", np.concatenate(recs["gres"]), pkg.GLB_RES.names),
                               ("rescue", sw, pkg.SW_RES.names)):
        idx = ld(f"{stage}_index").astype(np.int64)
        assert len(idx) == min(len(full), bench.DUMP_SAMPLE[stage]) and (np.diff(idx) > 0).all()
        fields = kswlib.SW_FIELDS if stage == "rescue" else names
        for f in fields:
            assert np.array_equal(ld(f"{stage}_{f}"), full[idx, names.index(f)].astype(np.float64)), (stage, f)
    # CIGAR words: the last chunk's sampled tasks, whole, in index order
    gidx = ld("global_index").astype(np.int64)
    last0 = chunks[0]["ng"]
    want, owner = [], []
    for t in gidx[gidx >= last0]:
        o, n = int(gtl["cigar_off"][t - last0]), int(recs["gres"][1][t - last0, 1])
        want.append(cig[o:o + n])
        owner += [t] * n
    assert np.array_equal(ld("global_cigar"), np.concatenate(want).astype(np.float64))
    assert np.array_equal(ld("global_cigar_task"), np.array(owner, np.float64))
    # same inputs, same files
    d2 = bench.dump_outputs(str(tmp_path / "b"), torch, pkg, kswlib, chunks, swb, d_cig, gtl)
    assert d2["files"] == d["files"]
    for f in d["files"]:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_dump_outputs_keep_to_the_budget(tmp_path, monkeypatch):
    """with a budget smaller than the sample the CIGAR words are cut (whole tasks), never the byte limit"""
    monkeypatch.setattr(bench, "DUMP_SAMPLE", {"seedext": 1000, "global": 800, "rescue": 10_000})
    chunks, swb, d_cig, gtl, recs, sw, cig = _case()
    full = bench.dump_outputs(str(tmp_path / "full"), torch, pkg, kswlib, chunks, swb, d_cig, gtl)
    words = len(np.load(tmp_path / "full" / "global_cigar.npy"))
    monkeypatch.setattr(bench, "DUMP_BYTES", full["bytes"] - 16 * (words // 2))
    d = bench.dump_outputs(str(tmp_path / "cut"), torch, pkg, kswlib, chunks, swb, d_cig, gtl)
    assert d["bytes"] <= bench.DUMP_BYTES
    got = np.load(tmp_path / "cut" / "global_cigar_task.npy")
    assert 0 < len(got) < words and np.array_equal(got, np.load(tmp_path / "full" / "global_cigar_task.npy")[:len(got)])
