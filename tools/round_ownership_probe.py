"""The cores after one round of each input of tests/test_round_ownership_gpu.py (chain, truncate, general, the two
rank-deficient cores, the doubled TT, the sharded decline), one .npy per core under OUTDIR, with the path taken; and, with
--bench-pool, the pool bytes after one warm-up round(256) at the bench shape (order 10, n = 20, rank 256).
Run it on two library builds (XRS_LIB_PATH) and compare the directories byte by byte:
    python tools/round_ownership_probe.py OUTDIR [--bench-pool]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import xerus_ref as ref   # noqa: E402
from xerus_amd import capi, dist as xd   # noqa: E402
import test_round_ownership_gpu as T   # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    h = capi.Handle(0)
    for name, (make, eps, _) in T.CASES.items():
        cores, target = make(ref)
        g = capi.TTDevice.from_cores(h, [c.copy() for c in cores])
        g.round(target, eps)
        print(name, h.last_round_path(), g.ranks, flush=True)
        for k, c in enumerate(g.cores()):
            np.save(os.path.join(out, f"{name}_{k}.npy"), c)
        g.free()
    d, world = 5, 3
    s = ref.tt_add(ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(51)), ref.TT.random_raw([1] * d, [2] * (d - 1), ref.Rng(52)))
    comm = xd.EmulatedComm(h, world)
    st = xd.ShardedTT(h, capi.TTDevice.from_cores(h, s.cores), [world] * d, world, 0)
    print("sharded-decline", repr(st.round_sharded(3, comm)), st.ranks, flush=True)
    for k, c in enumerate(st.local.cores()):
        np.save(os.path.join(out, f"sharded-decline_{k}.npy"), c)
    st.local.free()
    comm.close()
    h.close()
    if "--bench-pool" in sys.argv:
        h = capi.Handle(0)
        x = ref.TT.random_raw([20] * 10, [256] * 9, ref.Rng(23))
        g = capi.TTDevice.from_cores(h, x.cores)
        g.move_core(0)
        before = h.pool_bytes()
        g.round(256)
        print("bench shape: path", h.last_round_path(), "pool bytes before / after the warm-up round", before, h.pool_bytes(), flush=True)
        g.free()
        h.close()


if __name__ == "__main__":
    main()
