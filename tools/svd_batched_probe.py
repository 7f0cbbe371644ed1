"""xrs_svd_batched against a loop of xrs_svd calls on the same inputs (Gaussian members, preallocated outputs).

Per (shape, batch): one warm-up of each, then TRIALS alternating trials; a trial is the wall time of the whole
call (or the whole loop) between two stream synchronisations. Reported: median and [min, max] of each, the ratio
of the medians, and a verdict -- "wins" only if the batched call's slowest trial beats the loop's fastest one,
i.e. by more than the run-to-run spread of the two. The loop runs the single-matrix route unchanged.

    python tools/svd_batched_probe.py [--out FILE] [--trials N]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xerus_amd import capi  # noqa: E402
from xerus_amd.capi import _DP  # noqa: E402

SHAPES = [(16, 16), (32, 32), (64, 64), (32, 256)]
BATCHES = [1, 8, 64, 512]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trials", type=int, default=7)
    args = ap.parse_args()
    h = capi.Handle(0)
    lib = h.lib
    lines = ["# xrs_svd_batched vs a loop of xrs_svd; wall ms per whole batch, median [min, max] of %d alternating trials "
             "after one warm-up each" % args.trials,
             "# %-8s %5s  %-30s %-30s %8s  %s" % ("shape", "batch", "batched ms", "loop ms", "loop/bat", "verdict")]
    print("\n".join(lines), flush=True)
    for (m, n) in SHAPES:
        k = min(m, n)
        for batch in BATCHES:
            A = np.random.default_rng([m, n, batch]).standard_normal((batch, m, n))
            dA = h.array(A)
            U, S, Vt = h.empty((batch, m, k)), h.empty((batch, k)), h.empty((batch, k, n))
            U2, S2, Vt2 = h.empty((batch, m, k)), h.empty((batch, k)), h.empty((batch, k, n))
            st = np.zeros(batch, dtype=np.intc)

            def batched():
                capi._check("xrs_svd_batched", lib.xrs_svd_batched(h.h, _DP(U.ptr), _DP(S.ptr), _DP(Vt.ptr),
                                                                   st.ctypes.data_as(C.POINTER(C.c_int)), _DP(dA.ptr), batch, m, n))

            def loop():
                for b in range(batch):
                    capi._check("xrs_svd", lib.xrs_svd(h.h, _DP(U2.ptr + 8 * b * m * k), _DP(S2.ptr + 8 * b * k),
                                                       _DP(Vt2.ptr + 8 * b * k * n), _DP(dA.ptr + 8 * b * m * n), m, n))

            def timed(fn):
                h.synchronize()
                t0 = time.perf_counter()
                fn()
                h.synchronize()
                return (time.perf_counter() - t0) * 1e3

            batched()
            loop()
            fallbacks = int((st < 0).sum())
            # same inputs, same answer (singular values; the vectors are checked by tests/test_svd_batched_gpu.py)
            ds = np.abs(S.numpy() - S2.numpy()).max() / S2.numpy().max()
            tb, tl = [], []
            for _ in range(args.trials):
                tb.append(timed(batched))
                tl.append(timed(loop))
            mb, ml = float(np.median(tb)), float(np.median(tl))
            verdict = "wins" if max(tb) < min(tl) else ("loses" if min(tb) > max(tl) else "within spread")
            line = "%-10s %5d  %-30s %-30s %8.2f  %s (fallbacks %d, max dS %.1e)" % (
                "%dx%d" % (m, n), batch, "%.3f [%.3f, %.3f]" % (mb, min(tb), max(tb)),
                "%.3f [%.3f, %.3f]" % (ml, min(tl), max(tl)), ml / mb, verdict, fallbacks, ds)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    h.close()


if __name__ == "__main__":
    main()
