"""Reference values behind the bars of tests/test_chol_batch_gpu.py, on the CPU: the residuals of LAPACK's float64
Cholesky factor and inverse (well-conditioned cases) and of the float64 blocked emulation (graded cases), evaluated in
long double as the tests evaluate the device's. Prints, per group, the worst value of each quantity and the bar
8 x worst rounded up to a power of two (the tests cap a well-conditioned bar at 16 n u of the order at hand).
python tools/chol_bars.py [group ...]"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import chol_ref as cr  # noqa: E402


def bar(v):
    return 2.0 ** math.ceil(math.log2(8.0 * v)) if v > 0 else 0.0


def f64_shifted(A, shift):
    return A + shift * np.trace(A) * np.eye(A.shape[0]) if shift else A


def well_group(orders):
    worst = np.zeros(3)
    for n in orders:
        A, _ = cr.well(n)
        for shift in cr.SHIFTS:   # (a scale by a power of two changes no residual of the reference)
            As = cr.shifted(A, shift)
            L = np.linalg.cholesky(f64_shifted(A, shift))
            Z = np.linalg.inv(L)
            worst = np.maximum(worst, [cr.res_L(As, L), cr.res_Z(Z, L), cr.white(As, Z)])
    return worst


def graded_group(orders, nbs):
    worst = np.zeros(3)
    for n in orders:
        mats = {name: A for name, A, _ in cr.graded_cases(n)}
        for name, shift in cr.GRADED_JOBS:
            A = mats[name]
            As = cr.shifted(A, shift)
            for nb in nbs:
                L, Z = cr.blocked_chol_f64(f64_shifted(A, shift), nb)
                worst = np.maximum(worst, [cr.res_L(As, L), cr.res_Z(Z, L), cr.white(As, Z)])
    return worst


def trsm_group(orders):
    worst = 0.0
    for n in orders:
        A, _ = cr.well(n)
        L = np.linalg.cholesky(A)
        Y = cr.rhs(n)
        X = np.linalg.solve(L, Y)
        Xr = cr.forward_ld(L, Y)
        worst = max(worst, cr.factor_err(X, Xr))
    return worst


if __name__ == "__main__":
    only = sys.argv[1:]
    for name, orders in cr.WELL_GROUPS.items():
        if only and name not in only:
            continue
        w = well_group(orders)
        print("well   %-8s n %-28s worst res_L %.2e res_Z %.2e white %.2e   bars %s   (16 n u at the smallest n: %.2e)"
              % (name, orders, w[0], w[1], w[2], [bar(v) for v in w], 16 * min(orders) * cr.U), flush=True)
    for name, (orders, nbs) in cr.GRADED_GROUPS.items():
        if only and name not in only:
            continue
        w = graded_group(orders, nbs)
        print("graded %-8s n %-16s nb %-10s worst res_L %.2e res_Z %.2e white %.2e   bars %s"
              % (name, orders, nbs, w[0], w[1], w[2], [bar(v) for v in w]), flush=True)
    for name, orders in cr.TRSM_GROUPS.items():
        if only and name not in only:
            continue
        w = trsm_group(orders)
        print("trsm   %-8s n %-28s worst %.2e   bar %s" % (name, orders, w, bar(w)), flush=True)
