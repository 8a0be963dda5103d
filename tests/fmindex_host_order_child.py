"""Child process of tests/test_fmindex_launch_gpu.py::test_host_order_path_in_a_fresh_process.  BMH_SMEM_HOST_ORDER is
read once per process, so the host reorder path of smem_impl needs a process of its own that starts with it set: 1 000
reads through bmh_smem_batch and bmh_seed_batch, both kernels, against the oracle.  Exits non-zero on a mismatch."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import kswlib  # noqa: E402
from test_fmindex_cpu import _intv_len, _orc_calls, _same_calls, fixture_reads  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    if os.environ.get("BMH_SMEM_HOST_ORDER") != "1":
        print("BMH_SMEM_HOST_ORDER=1 is not set")
        return 2
    cb, keep, raw, opt, reads, per, sa_k, sa_pos = kswlib.golden_fmindex()
    more = fixture_reads(223, 1000, [1, 18, 19, 20, 75, 150, 151, 300], [0.0, 0.02, 0.12])
    more[7], more[500] = np.zeros(0, np.uint8), np.full(30, 4, np.uint8)
    bad = 0
    for oname in ("fixture", "eager"):
        o = kswlib.smem_option_set(oname)
        want = [_orc_calls(cb, o, rd) for rd in more]
        for kernel in ("conv", "loops"):
            os.environ["BMH_SMEM_KERNEL"] = kernel
            ctx = load_package().Context(0, kswlib.make_params())
            ctx.set_bwt(*raw)
            got = ctx.smem_batch(o, more)
            seeded, offs, pos = ctx.seed_batch(o, 50, more)
            ctx.close()
            keys, have = [], []
            for r, (g, s, so, w) in enumerate(zip(got, seeded, offs, want)):
                if not (_same_calls(g, w) and _same_calls(s, w)):
                    bad += 1
                    print(f"MISMATCH {oname} {kernel} read {r} (len {len(more[r])})")
                    continue
                iv = w[1]
                look = (_intv_len(iv) >= int(o["min_seed_len"])) & (iv["x2"] <= np.uint64(50))
                if not ((so != np.uint64(0xffffffffffffffff)) == look).all():
                    bad += 1
                    print(f"LOOK-UP SET {oname} {kernel} read {r}")
                    continue
                for k in np.nonzero(look)[0]:
                    x0, x2, b = int(iv["x0"][k]), int(iv["x2"][k]), int(so[k])
                    keys.append(np.arange(x0, x0 + x2, dtype=np.uint64))
                    have.append(pos[b:b + x2])
            keys, have = np.concatenate(keys), np.concatenate(have)
            if len(keys) < 1000 or len(keys) != len(pos) or len(have) != len(keys) or not (have == kswlib.orc_sa(cb, keys)).all():
                bad += 1
                print(f"POSITIONS {oname} {kernel}: {len(keys)} keys, {len(pos)} positions")
    print("mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
