"""Matrix-free ALS probe: the dense local solve against the matrix-free one, and the matrix-free one
alone at ranks the dense path cannot reach.

  dense vs matrix-free   xe.ALS_SPD against xe.ALS_SPD_MF on the Laplace operator, d = 8, n = 8, x of rank 24 (interior
                         local systems of order 24 * 8 * 24 = 4608; the dense operator has 170 MB): wall clock of a run of
                         two half sweeps from the same start (environment stacks included), halved; the two alternate
                         after a warm-up of each, median of --reps (min .. max); the final energies beside the times.
  matrix-free alone      xe.ALS_SPD_MF at r = 64 and r = 128 (the dense operator would have 8.6 GB / 137 GB): the same
                         wall clock, and the local solve of the middle site through the C-ABI (environments of
                         orthonormal random cores from numpy) under xrs_prof_begin / xrs_prof_end: CG iterations, kernel
                         launches per iteration (GEMM chain, split-K reduces and the three CG kernels) and kernel time per
                         iteration.

    python tools/als_local_probe.py [--reps 7] [--ranks 64,128] [--skip compare,alone]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xerus_amd import capi  # noqa: E402

D, N_MODE = 8, 8


def laplace_cores(d, n):
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    I = np.eye(n)
    cs = []
    for k in range(d):
        c = np.zeros((1 if k == 0 else 2, n, n, 1 if k == d - 1 else 2))
        if k == 0:
            c[0, :, :, 0], c[0, :, :, 1] = T, I
        elif k == d - 1:
            c[0, :, :, 0], c[1, :, :, 0] = I, T
        else:
            c[0, :, :, 0], c[1, :, :, 0], c[1, :, :, 1] = I, T, I
        cs.append(c)
    return cs


def operator(xe, cores):
    A = xe.TTOperator([c.shape[1] for c in cores] + [c.shape[2] for c in cores])
    for k, c in enumerate(cores):
        A.set_component(k, xe.Tensor.from_ndarray(np.ascontiguousarray(c)))
    return A


def half_sweep_ms(xe, variant, A, x0, b):
    x = xe.TTTensor(x0)
    xe.synchronize()
    t0 = time.perf_counter()
    energy = variant(A, x, b, 2)
    xe.synchronize()
    return (time.perf_counter() - t0) * 1e3 / 2, energy


def timed(xe, variants, A, x0, b, reps):
    """median (min, max) ms per half sweep and the last energy of each variant, alternating after a warm-up of each"""
    ms = [[] for _ in variants]
    en = [None] * len(variants)
    for rep in range(reps + 1):
        for k, v in enumerate(variants):
            t, en[k] = half_sweep_ms(xe, v, A, x0, b)
            if rep:
                ms[k].append(t)
    return [(statistics.median(t), min(t), max(t), e) for t, e in zip(ms, en)]


def setup(xe, r):
    xe.seed(4242 + r)
    A = operator(xe, laplace_cores(D, N_MODE))
    b = xe.TTTensor.random([N_MODE] * D, [2] * (D - 1))
    x0 = xe.TTTensor.random([N_MODE] * D, [r] * (D - 1))
    return A, x0, b


def compare(reps):
    import xerus_amd.xerus as xe

    r = 24
    A, x0, b = setup(xe, r)
    (d_ms, d_lo, d_hi, d_en), (m_ms, m_lo, m_hi, m_en) = timed(xe, [xe.ALS_SPD, xe.ALS_SPD_MF], A, x0, b, reps)
    print(f"dense vs matrix-free: Laplace, d = {D}, n = {N_MODE}, r = {r} (ranks {x0.ranks()}), ms per half sweep, "
          f"median of {reps} (min .. max)")
    print(f"  ALS_SPD    (dense local operator + Cholesky) : {d_ms:9.2f} ({d_lo:9.2f} .. {d_hi:9.2f})   energy {d_en:.12e}")
    print(f"  ALS_SPD_MF (GEMM chain + device CG)          : {m_ms:9.2f} ({m_lo:9.2f} .. {m_hi:9.2f})   energy {m_en:.12e}")
    print(f"  dense / matrix-free = {d_ms / m_ms:.2f}", flush=True)


def middle_site_problem(r, rng):
    """(dims, L, A, R, x0, b) of site D / 2 for orthonormal random cores of rank r (capped by the mode sizes)."""
    cores = laplace_cores(D, N_MODE)
    ranks = [1] + [min(r, N_MODE ** min(k, D - k)) for k in range(1, D)] + [1]
    site = D // 2
    L = np.ones((1, 1, 1))
    for k in range(site):
        Q = np.linalg.qr(rng.standard_normal((ranks[k] * N_MODE, ranks[k + 1])))[0].reshape(ranks[k], N_MODE, ranks[k + 1])
        L = np.einsum('pqr,pnc,qnmd,rme->cde', L, Q, cores[k], Q, optimize=True)
    R = np.ones((1, 1, 1))
    for k in range(D - 1, site, -1):
        Q = np.linalg.qr(rng.standard_normal((N_MODE * ranks[k + 1], ranks[k])))[0].T.reshape(ranks[k], N_MODE, ranks[k + 1])
        R = np.einsum('pnc,qnmd,rme,cde->pqr', Q, cores[k], Q, R, optimize=True)
    rl, rr = ranks[site], ranks[site + 1]
    A = cores[site]
    dims = (rl, N_MODE, rr, A.shape[0], A.shape[3])
    return dims, L, A, R, rng.standard_normal((rl, N_MODE, rr)), rng.standard_normal((rl, N_MODE, rr))


def alone(reps, ranks):
    import xerus_amd.xerus as xe

    mask = capi.KFAM_GEMM | capi.KFAM_PERMUTE | capi.KFAM_ELEMWISE | capi.KFAM_SPLITK
    print(f"matrix-free alone: Laplace, d = {D}, n = {N_MODE}; local solve of site {D // 2} to 1e-12 under xrs_prof_begin/end")
    for r in ranks:
        A, x0, b = setup(xe, r)
        (ms, lo, hi, en), = timed(xe, [xe.ALS_SPD_MF], A, x0, b, reps)
        print(f"  r = {r:4d} (ranks {x0.ranks()}): ALS_SPD_MF {ms:9.2f} ({lo:9.2f} .. {hi:9.2f}) ms per half sweep, energy {en:.12e}")
        dims, L, Ac, R, xs, bs = middle_site_problem(r, np.random.default_rng(r))
        h = capi.Handle(0)
        dL, dA, dR, db = h.array(L), h.array(Ac), h.array(R), h.array(bs)
        h.als_local_cg(h.array(xs), db, dims, dL, dA, dR, False, 1e-12, 0, 16)   # warm-up
        dx = h.array(xs)
        h.prof_begin(mask)
        iters, relres, status = h.als_local_cg(dx, db, dims, dL, dA, dR, False, 1e-12, 0, 16)
        prof = h.prof_end()
        h.synchronize()
        t0 = time.perf_counter()
        h.als_local_cg(h.array(xs), db, dims, dL, dA, dR, False, 1e-12, 0, 16)
        wall = (time.perf_counter() - t0) * 1e3
        enq = -(-iters // 16) * 16   # iterations enqueued: up to the host's next look
        print(f"           site {D // 2}: N = {dims[0] * dims[1] * dims[2]}, status {status}, {iters} CG iterations ({enq} enqueued), "
              f"relres {relres:.2e}; {prof['launches']} launches = {(prof['launches'] - 6) / enq:.2f} per enqueued iteration, "
              f"kernel time {prof['ms']:.3f} ms = {prof['ms'] / enq * 1e3:.1f} us per iteration; wall {wall:.2f} ms", flush=True)
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ranks", default="64,128")
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    if "compare" not in skip:
        compare(a.reps)
    if "alone" not in skip:
        alone(a.reps, [int(v) for v in a.ranks.split(",")])


if __name__ == "__main__":
    main()
