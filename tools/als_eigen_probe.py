"""ALS_EIGEN probe: the matrix-free eigen sweep beside the matrix-free linear solve it shares the local
GEMM chain with. A record, not a bar.

  half sweeps   xe.ALS_EIGEN against xe.ALS_SPD_MF on the Laplace operator, d = 8, n = 8, at r = 24, 64 and 128, from
                the same start: wall clock of a run of two half sweeps (environment stacks included), halved; the two
                alternate after a warm-up of each, median of --reps (min .. max); lambda / the energy beside the times.
  middle site   the local eigenproblem of site d / 2 through the C-ABI (environments of orthonormal random cores from
                numpy, the setup of als_local_probe.py) to 1e-10 under xrs_prof_begin / xrs_prof_end: LOBPCG
                iterations, kernel launches per enqueued iteration (the GEMM chain with its split-K reduces, its
                length solved from the profiled total, and the three vector kernels) and kernel time per iteration; the CG of the same site to 1e-10 for comparison.

    python tools/als_eigen_probe.py [--reps 7] [--ranks 24,64,128]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from als_local_probe import D, N_MODE, middle_site_problem, setup  # noqa: E402
from xerus_amd import capi  # noqa: E402

# launches of a solve = 1 (the core permutation) + the initialisation's vector kernels + one chain
#                      + enqueued iterations x (one chain + 3 vector kernels);
# a chain is 3 GEMMs plus their split-K reduces, whose number depends on r, so its length is solved from the total
INIT_VECTOR_EIG, INIT_VECTOR_CG, ITER_VECTOR = 5, 2, 3


def per_iteration(launches, init_vector, enq):
    """(launches per enqueued iteration, launches of one chain) from the profiled total; the chain length must come
    out whole."""
    chain, rest = divmod(launches - 1 - init_vector - ITER_VECTOR * enq, enq + 1)
    if rest:
        raise RuntimeError(f"{launches} launches do not split into {enq} iterations and one initial chain")
    return chain + ITER_VECTOR, chain


def half_sweep_ms(xe, run, x0):
    x = xe.TTTensor(x0)
    xe.synchronize()
    t0 = time.perf_counter()
    value = run(x)
    xe.synchronize()
    return (time.perf_counter() - t0) * 1e3 / 2, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ranks", default="24,64,128")
    a = ap.parse_args()
    import xerus_amd.xerus as xe

    mask = capi.KFAM_GEMM | capi.KFAM_PERMUTE | capi.KFAM_ELEMWISE | capi.KFAM_SPLITK
    print(f"ALS_EIGEN vs ALS_SPD_MF: Laplace, d = {D}, n = {N_MODE}; ms per half sweep, median of {a.reps} (min .. max); "
          f"site {D // 2} alone to 1e-10 under xrs_prof_begin/end")
    for r in [int(v) for v in a.ranks.split(",")]:
        A, x0, b = setup(xe, r)
        runs = [lambda x: xe.ALS_EIGEN(A, x, 2), lambda x: xe.ALS_SPD_MF(A, x, b, 2)]
        ms, val = [[], []], [None, None]
        for rep in range(a.reps + 1):
            for k, run in enumerate(runs):
                t, val[k] = half_sweep_ms(xe, run, x0)
                if rep:
                    ms[k].append(t)
        print(f"  r = {r:4d} (ranks {x0.ranks()})")
        for name, t, v, what in (("ALS_EIGEN ", ms[0], val[0], "lambda"), ("ALS_SPD_MF", ms[1], val[1], "energy")):
            print(f"    {name} {statistics.median(t):9.2f} ({min(t):9.2f} .. {max(t):9.2f})   {what} {v:.12e}")
        dims, L, Ac, R, xs, bs = middle_site_problem(r, np.random.default_rng(r))
        h = capi.Handle(0)
        dL, dA, dR, db = h.array(L), h.array(Ac), h.array(R), h.array(bs)
        for name, init, solve in (("LOBPCG", INIT_VECTOR_EIG, lambda x: h.als_local_eig(x, dims, dL, dA, dR, 1e-10, 0, 16)[1:]),
                                  ("CG    ", INIT_VECTOR_CG, lambda x: h.als_local_cg(x, db, dims, dL, dA, dR, False, 1e-10, 0, 16))):
            solve(h.array(xs))   # warm-up
            dx = h.array(xs)
            h.prof_begin(mask)
            iters, relres, status = solve(dx)
            prof = h.prof_end()
            h.synchronize()
            t0 = time.perf_counter()
            solve(h.array(xs))
            wall = (time.perf_counter() - t0) * 1e3
            enq = max(16, -(-iters // 16) * 16)   # iterations enqueued: up to the host's next look
            per, chain = per_iteration(prof['launches'], init, enq)
            print(f"    site {D // 2} {name}: N = {dims[0] * dims[1] * dims[2]}, status {status}, {iters} iterations ({enq} enqueued), "
                  f"relres {relres:.2e}; {prof['launches']} launches = {per} per enqueued iteration (chain {chain}), "
                  f"kernel time {prof['ms']:.3f} ms = {prof['ms'] / enq * 1e3:.1f} us per iteration; wall {wall:.2f} ms", flush=True)
        h.close()


if __name__ == "__main__":
    main()
