"""UQ-ADF probe: one full sweep of uq_adf and the per-sample congruence kernel alone, at
N = 20000, d = 6, n_0 = 1000, n_k = 8 with all ranks 32 and with all ranks 8 (TTTensor::random caps the last
rank at n_5 = 8; the ranks used are printed).

  - ms per sweep: (time of 3 iterations - time of 1 iteration) / 2 through the extended uq_adf overload, so the
    one-off upload of the samples drops out; wall clock around calls that end synchronised, median of --reps;
  - the congruence kernel alone (xrs_uq_stack_congruence, a = b = rank, with an L stack): HIP events on the
    handle's stream, median of --reps after a warm-up; its byte floor N (a^2 + b^2) 8 B at the HBM rate a copy
    kernel reaches on this part (6.29 TB/s) and at the 8 TB/s of the data sheet;
  - for rank 32 the same launch forced onto the MFMA and onto the FMA kernel (XRS_UQ_CONGRUENCE).

    python tools/uq_probe.py [--N 20000 --reps 7] [--kernel-only]
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
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def _hip(status):
    if status != 0:
        raise RuntimeError(f"HIP call failed with status {status}")


def kernel_ms(h, fn, reps):
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    _hip(hip.hipEventCreate(ctypes.byref(start)))
    _hip(hip.hipEventCreate(ctypes.byref(stop)))
    stream = ctypes.c_void_p(h.stream())
    fn()
    h.synchronize()
    times = []
    for _ in range(reps):
        _hip(hip.hipEventRecord(start, stream))
        fn()
        _hip(hip.hipEventRecord(stop, stream))
        _hip(hip.hipEventSynchronize(stop))
        ms = ctypes.c_float()
        _hip(hip.hipEventElapsedTime(ctypes.byref(ms), start, stop))
        times.append(ms.value)
    return statistics.median(times), min(times), max(times)


def congruence_alone(h, N, rank, n, reps, force=None):
    rng = np.random.default_rng(rank)
    X = h.array(rng.standard_normal((rank, n, rank)) / np.sqrt(rank * n))
    P = h.array(rng.standard_normal((N, n)))
    G = rng.standard_normal((rank, rank))
    L = h.array(np.broadcast_to(G @ G.T, (N, rank, rank)))
    out = h.empty((N, rank, rank))
    lib = h.lib
    if force:
        os.environ["XRS_UQ_CONGRUENCE"] = force
    else:
        os.environ.pop("XRS_UQ_CONGRUENCE", None)

    def run():
        st = lib.xrs_uq_stack_congruence(h.h, ctypes.c_void_p(out.ptr), ctypes.c_void_p(L.ptr), ctypes.c_void_p(X.ptr),
                                         ctypes.c_void_p(P.ptr), N, rank, n, rank)
        if st != 0:
            raise RuntimeError(lib.xrs_last_error().decode())

    med, lo, hi = kernel_ms(h, run, reps)
    os.environ.pop("XRS_UQ_CONGRUENCE", None)
    floor_bytes = N * 2 * rank * rank * 8
    label = {None: "by shape", "mfma": "MFMA forced", "fma": "FMA forced"}[force]
    print(f"congruence alone, rank {rank:3d}, n {n}, N {N} ({label:11s}): median {med:8.4f} ms (min {lo:.4f}, max {hi:.4f}); "
          f"floor {floor_bytes / 1e6:.1f} MB = {floor_bytes / HBM_MEASURED * 1e3:.4f} ms at 6.29 TB/s: "
          f"{floor_bytes / HBM_MEASURED * 1e3 / med:.3f} of it ({floor_bytes / HBM_SPEC * 1e3 / med:.3f} at 8 TB/s)")
    return med


def sweep(N, rank, reps):
    import xerus_amd.xerus as xe

    dims = [1000, 8, 8, 8, 8, 8]
    xe.seed(1234)
    true = xe.TTTensor.random(dims, [rank] * 5)
    true = true / true.frob_norm()
    rv, sols = xe.uq_mc(true, N, 0)   # samples of a target of these ranks
    start = xe.TTTensor.random(dims, [rank] * 5)
    start = start / start.frob_norm()   # the target's scale: a start far off it ends the solver's first check

    def run(iters):
        x = xe.TTTensor(start)
        xe.synchronize()
        t = time.perf_counter()
        hist = xe.uq_adf(x, rv, sols, iters)
        xe.synchronize()
        return (time.perf_counter() - t) * 1e3, len(hist)

    run(1)
    per = []
    for _ in range(reps):
        t1, n1 = run(1)
        t3, n3 = run(3)
        if n3 != 3:
            raise RuntimeError("the solver stopped before three iterations")
        per.append((t3 - t1) / 2)
    print(f"uq_adf sweep, ranks {true.ranks()}, N {N}, dims {dims}: median {statistics.median(per):9.3f} ms per sweep "
          f"(min {min(per):.3f}, max {max(per):.3f}, {reps} runs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    h = capi.Handle(0)
    for rank in (32, 8):
        congruence_alone(h, a.N, rank, 8, a.reps)
    mf = congruence_alone(h, a.N, 32, 8, a.reps, "mfma")
    fm = congruence_alone(h, a.N, 32, 8, a.reps, "fma")
    print(f"rank 32 A/B: MFMA {mf:.4f} ms, FMA {fm:.4f} ms: MFMA / FMA = {mf / fm:.3f}")
    for rank in (16, 24, 48, 64):
        m = congruence_alone(h, a.N, rank, 8, a.reps, "mfma")
        f = congruence_alone(h, a.N, rank, 8, a.reps, "fma")
        print(f"rank {rank} A/B: MFMA / FMA = {m / f:.3f}")
    h.close()
    if not a.kernel_only:
        for rank in (32, 8):
            sweep(a.N, rank, max(3, a.reps // 2))


if __name__ == "__main__":
    main()
