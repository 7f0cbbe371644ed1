"""Randomized rounding probe: xe.sum_rounded against operator+ followed by round of the same build, and
xrs_gemm_ksum against a loop of xrs_gemm + xrs_axpy.

  end to end   the benchmark's cfg3 shape: order 10, n = 20, two random rank-128 terms rounded to 128, oversampling 8
               and 16. (x + y).round(128) and xe.sum_rounded([x, y], [1, 1], ranks, oversampling) alternate after one
               warm-up of each; wall clock around calls that end synchronised; median [min, max] of --reps trials.
               Beside the times: the relative error of each result against x + y and of the two results against each
               other (TT arithmetic: ||a - b|| from the rounded difference's core).
  kernel       the pass-2 products of that shape, Z ((l n) x l) = sum_j V(X_j) (l n x 128) W_j (128 x l), l = 128 + p,
               for 2, 3 and 8 terms: one xrs_gemm_ksum against xrs_gemm into C, then xrs_gemm into a scratch and
               xrs_axpy per further term. HIP events around --inner back-to-back calls, alternating, median [min, max]
               of --reps after one warm-up of each; the two results' largest elementwise difference beside them.

    python tools/rand_round_probe.py [--reps 7] [--inner 10] [--skip e2e,kernel]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xerus_amd import capi  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")


def _hip(status):
    if status != 0:
        raise RuntimeError(f"HIP call failed with status {status}")


def event_ms(h, fns, reps, inner):
    """(median, min, max) of the time per call of the callables in fns, run alternately in groups of `inner` calls
    after one warm-up of each."""
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    _hip(hip.hipEventCreate(ctypes.byref(start)))
    _hip(hip.hipEventCreate(ctypes.byref(stop)))
    stream = ctypes.c_void_p(h.stream())
    for fn in fns:
        fn()
    h.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            _hip(hip.hipEventRecord(start, stream))
            for _ in range(inner):
                fn()
            _hip(hip.hipEventRecord(stop, stream))
            _hip(hip.hipEventSynchronize(stop))
            ms = ctypes.c_float()
            _hip(hip.hipEventElapsedTime(ctypes.byref(ms), start, stop))
            times[k].append(ms.value / inner)
    _hip(hip.hipEventDestroy(start))
    _hip(hip.hipEventDestroy(stop))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def fmt(t):
    return f"{statistics.median(t):8.3f} [{min(t):8.3f}, {max(t):8.3f}]"


def end_to_end(reps):
    import xerus_amd.xerus as xe

    d, n, rank = 10, 20, 128
    xe.seed(0xC0FFEE)
    x, y = xe.TTTensor.random([n] * d, rank), xe.TTTensor.random([n] * d, rank)
    ranks = [rank] * (d - 1)
    exact = x + y
    norm = exact.frob_norm()

    def wall(fn):
        xe.synchronize()
        t0 = time.perf_counter()
        out = fn()
        xe.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def plus_round():
        s = x + y
        s.round(rank)
        return s

    def dist(a, b):
        diff = a - b
        diff.move_core(0)
        return diff.frob_norm()

    print(f"end to end: order {d}, n = {n}, two rank-{rank} terms -> {rank}; ms per call, median [min, max] of {reps} "
          f"alternating trials after one warm-up", flush=True)
    for p in (8, 16):
        over = [p] * (d - 1)
        rnd = lambda: xe.sum_rounded([x, y], [1.0, 1.0], ranks, over)  # noqa: E731
        ta, tb = [], []
        a = b = None
        for rep in range(reps + 1):
            ms_a, a = wall(plus_round)
            ms_b, b = wall(rnd)
            if rep:
                ta.append(ms_a)
                tb.append(ms_b)
        print(f"  oversampling {p:2d}: (x + y).round({rank}) {fmt(ta)}   sum_rounded {fmt(tb)}   ratio {statistics.median(ta) / statistics.median(tb):.2f}")
        print(f"                   relative error against x + y: round {dist(a, exact) / norm:.4e}, sum_rounded {dist(b, exact) / norm:.4e}; "
              f"between the two results {dist(a, b) / a.frob_norm():.4e}; ranks {b.ranks()}", flush=True)


def kernel(reps, inner):
    h = capi.Handle(0)
    rng = np.random.default_rng(0)
    n, R = 20, 128
    print(f"kernel: Z ((l n) x l) = sum_j X_j ((l n) x {R}) W_j ({R} x l), n = {n}; ms per product, median [min, max] of {reps} "
          f"after one warm-up, HIP events around {inner} calls", flush=True)
    for p in (8, 16):
        l = R + p
        M, N = l * n, l
        for s in (2, 3, 8):
            X = [h.array(rng.standard_normal((M, R))) for _ in range(s)]
            W = [h.array(rng.standard_normal((R, N))) for _ in range(s)]
            Z1, Z2, T = h.empty((M, N)), h.empty((M, N)), h.empty((M * N,))
            Z2flat = capi.DeviceArray(h, (M * N,), ptr=Z2.ptr, owned=False)

            def ksum():
                h.gemm_ksum(Z1, M, N, 1.0, X, W)

            def loop():
                h.gemm(Z2, M, N, 1.0, X[0], R, False, R, W[0], N, False)
                for j in range(1, s):
                    h.gemm(T, M, N, 1.0, X[j], R, False, R, W[j], N, False)
                    h.axpy(Z2flat, 1.0, T)

            (a, al, ah), (b, bl, bh) = event_ms(h, [ksum, loop], reps, inner)
            diff = np.abs(Z1.numpy() - Z2.numpy()).max()
            flops = 2.0 * M * N * R * s
            print(f"  l = {l}, {M} x {N}, {s} terms: gemm_ksum {a:7.4f} [{al:7.4f}, {ah:7.4f}] ({flops / a / 1e9:6.2f} TF/s)   "
                  f"gemm + axpy loop {b:7.4f} [{bl:7.4f}, {bh:7.4f}]   loop / ksum {b / a:5.2f}   max |difference| {diff:.2e}", flush=True)
            for arr in X + W + [Z1, Z2, T]:
                arr.free()
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    if "kernel" not in skip:
        kernel(a.reps, a.inner)
    if "e2e" not in skip:
        end_to_end(a.reps)


if __name__ == "__main__":
    main()
