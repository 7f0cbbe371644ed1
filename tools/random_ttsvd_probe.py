"""Randomized TT-SVD probe: the two routes of xrs_sketch_gaussian against each other, and xe.randomTTSVD against
the TT-SVD constructor end to end.

  sketch routes   Y = G A for s in {16, 40, 72} sketch rows and n in {16, 64, 256, 1024} columns, m such that A has
                  --mib MiB (default 128): route 1 (fused: G generated inside the product) and route 2 (materialised:
                  xrs_gaussian_matrix into scratch, then xrs_gemm) alternate after a warm-up of each; HIP events on the
                  handle's stream around --inner back-to-back calls (so the queue stays fed and the host's enqueue
                  time drops out), divided by --inner; median of --reps. Beside each time: the bytes of A alone
                  over that time.
  end to end      xe.TTTensor(X, EPSILON, ranks) against xe.randomTTSVD(X, ranks, oversampling 8) with ranks 32 on
                    (a) dims 16^5, X a normalised random rank-32 TT plus 1e-4 relative noise,
                    (b) dims 16^6, the same construction,
                    (c) dims 16^5, X of exact rank 8 (no noise): every sketch is rank deficient, so xrs_rq takes its
                        Householder route;
                  wall clock around calls that end synchronised, alternating after a warm-up of each, median of
                  --e2e-reps; both relative errors beside the times.

    python tools/random_ttsvd_probe.py [--mib 128] [--reps 9] [--inner 10] [--e2e-reps 3] [--skip sketch,e2e,small,large]
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
    """Medians (and min, max) of the time per call of the callables in fns, run alternately in groups of `inner`
    calls; each is warmed up once first."""
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


def sketch_routes(mib, reps, inner):
    h = capi.Handle(0)
    print(f"sketch routes: Y (s x n) = G (s x m) A (m x n), A of {mib} MiB, median of {reps} (min .. max), HIP events around {inner} calls")
    print(f"{'s':>4} {'n':>5} {'m':>8} | {'fused ms':>24} {'A TB/s':>7} | {'materialised ms':>24} {'A TB/s':>7} | fused / mat. | auto")
    rng = np.random.default_rng(0)
    for n in (16, 64, 256, 1024):
        m = mib * 2 ** 20 // (8 * n)
        dA = h.array(rng.standard_normal((m, n)))
        a_bytes = 8.0 * m * n
        for s in (16, 40, 72):
            Y = h.empty((s, n))
            fused = lambda: h.sketch_gaussian(s, dA, 1, 2, route=1, out=Y)  # noqa: E731
            mat = lambda: h.sketch_gaussian(s, dA, 1, 2, route=2, out=Y)  # noqa: E731
            (f, fl, fh), (g, gl, gh) = event_ms(h, [fused, mat], reps, inner)
            h.sketch_gaussian(s, dA, 1, 2, route=0, out=Y)
            print(f"{s:>4} {n:>5} {m:>8} | {f:8.3f} ({fl:6.3f} .. {fh:6.3f}) {a_bytes / f / 1e9:7.2f} | "
                  f"{g:8.3f} ({gl:6.3f} .. {gh:6.3f}) {a_bytes / g / 1e9:7.2f} | {f / g:12.2f} | {h.sketch_last_route()}", flush=True)
            Y.free()
        dA.free()
    h.close()


def wall_ms(fn):
    import xerus_amd.xerus as xe

    xe.synchronize()
    t0 = time.perf_counter()
    out = fn()
    xe.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def end_to_end(name, dims, tt_rank, noise, reps):
    import xerus_amd.xerus as xe

    d = len(dims)
    xe.seed(4242 + d + tt_rank)
    x = xe.Tensor(xe.TTTensor.random(dims, tt_rank)).to_ndarray()
    x /= np.linalg.norm(x)
    if noise:
        x += noise / np.sqrt(x.size) * np.random.default_rng(d).standard_normal(x.shape)
    X = xe.Tensor.from_ndarray(x)
    ranks, over = [32] * (d - 1), [8] * (d - 1)
    eps = 8 * np.finfo(float).eps
    svd = lambda: xe.TTTensor(X, eps, ranks)  # noqa: E731
    rnd = lambda: xe.randomTTSVD(X, ranks, over)  # noqa: E731
    print(f"{name}: dims {dims[0]}^{d}, X of TT rank {tt_rank} + {noise:g} relative noise, ranks 32, oversampling 8", flush=True)
    ts, tr = [], []
    a = b = None
    for rep in range(reps + 1):   # the first pass is the warm-up
        ms_a, a = wall_ms(svd)
        ms_b, b = wall_ms(rnd)
        if rep:
            ts.append(ms_a)
            tr.append(ms_b)
        print(f"  pass {rep}: TT-SVD {ms_a:10.2f} ms, randomTTSVD {ms_b:10.2f} ms" + ("  (warm-up)" if rep == 0 else ""), flush=True)
    err = lambda t: np.linalg.norm(xe.Tensor(t).to_ndarray() - x) / np.linalg.norm(x)  # noqa: E731
    print(f"  TT-SVD      : median {statistics.median(ts):10.2f} ms, ranks {a.ranks()}, relative error {err(a):.3e}")
    print(f"  randomTTSVD : median {statistics.median(tr):10.2f} ms, ranks {b.ranks()}, relative error {err(b):.3e}")
    print(f"  TT-SVD / randomTTSVD = {statistics.median(ts) / statistics.median(tr):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    if "sketch" not in skip:
        sketch_routes(a.mib, a.reps, a.inner)
    if "e2e" not in skip:
        if "small" not in skip:
            end_to_end("(a)", [16] * 5, 32, 1e-4, a.e2e_reps)
            end_to_end("(c)", [16] * 5, 8, 0.0, a.e2e_reps)
        if "large" not in skip:
            end_to_end("(b)", [16] * 6, 32, 1e-4, a.e2e_reps)


if __name__ == "__main__":
    main()
