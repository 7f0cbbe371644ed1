"""CPU reference of the batched Cholesky family (csrc/smallla.hip k_potrf*, k_trsm16, k_trinv_batched; csrc/chol_batch.hip;
csrc/solve.hip chol_full): a long-double column Cholesky that reads the lower triangle only, the test matrices with
prescribed spectra or a prescribed first failing column, a float64 emulation of the blocked algorithm class the kernels
belong to, and the residuals the tests assert, all evaluated in long double (64-bit mantissa: u_ld = 5.4e-20)."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53            # unit roundoff of float64
TAU = 1.0e-11             # kGramShift: a certificate factors A - TAU tr(A) I
PIVOT_MAX = 1.0e300       # the kernels' pivot rule: 0 < pivot < 1e300


def mm(a, b):
    """a @ b in long double (numpy's long-double product is an order of magnitude faster on a Fortran-ordered b)."""
    return np.dot(np.asarray(a, dtype=LD), np.asfortranarray(np.asarray(b, dtype=LD)))


def tmm(x, y, x_lower=False, y_lower=False, y_upper=False, lower_only=False, nb=128):
    """x @ y in long double, skipping the blocks that a lower-triangular x, a lower- or upper-triangular y leave zero;
    lower_only: only the blocks on and below the diagonal of the (square) result are formed, the others left zero."""
    x, y = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    (m, K), n = x.shape, y.shape[1]
    out = np.zeros((m, n), dtype=LD)
    for i0 in range(0, m, nb):
        i1 = min(i0 + nb, m)
        for j0 in range(0, min(i1, n) if lower_only else n, nb):
            j1 = min(j0 + nb, n)
            lo = j0 if y_lower else 0
            hi = min(i1 if x_lower else K, j1 if y_upper else K)
            if lo < hi:
                out[i0:i1, j0:j1] = np.dot(np.ascontiguousarray(x[i0:i1, lo:hi]), np.asfortranarray(y[lo:hi, j0:j1]))
    return out


def shifted(A, shift_rel):
    """A + shift_rel tr(A) I in long double from the lower triangle of the float64 A (mirrored)."""
    W = np.tril(np.asarray(A, dtype=np.float64)).astype(LD)
    W = W + np.tril(W, -1).T
    tr = W.diagonal().sum()
    W[np.diag_indices_from(W)] += LD(shift_rel) * tr
    return W


def chol_ld(A, shift_rel=0.0):
    """Column Cholesky in long double of the float64 matrix A + shift_rel tr(A) I, reading the lower triangle only.
    Returns (L, status, pivots / tr A): status 0, or 1 + the first column whose pivot is not in (0, 1e300), where the
    factorisation stops (later pivots and columns of L are NaN)."""
    with np.errstate(all="ignore"):
        A = np.asarray(A, dtype=np.float64)
        n = A.shape[0]
        W = np.tril(A).astype(LD)
        tr = W.diagonal().sum()
        W[np.diag_indices(n)] += LD(shift_rel) * tr
        L = np.zeros((n, n), dtype=LD)
        piv = np.full(n, np.nan, dtype=LD)
        status = 0
        for k in range(n):
            c = W[k:, k] - np.dot(L[k:, :k], L[k, :k])
            piv[k] = c[0]
            if not (c[0] > 0 and c[0] < PIVOT_MAX):
                status = k + 1
                L[k:, k:] = np.where(np.tril(np.ones((n - k, n - k), dtype=bool)), np.nan, 0.0)
                break
            L[k:, k] = c / np.sqrt(c[0])
        return L, status, piv / tr


def _orth(n, seed):
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(R.diagonal())


def spd(n, lam, seed):
    """Q diag(lam) Q^T formed in long double (Q a float64 orthogonal factor), symmetrised, rounded to float64. The
    eigenvalues are lam up to a relative 1e-15 (Q's defect from orthogonality acts multiplicatively) and an absolute
    u max(lam) from the rounding."""
    Q = _orth(n, seed).astype(LD)
    lam = np.asarray(lam, dtype=LD)
    A = mm(Q * lam, Q.T)
    return ((A + A.T) / 2).astype(np.float64)


def graded(n, kappa):
    """n eigenvalues from 1 down to 1 / kappa, geometrically spaced (n = 1: just 1)."""
    return np.geomspace(1.0, 1.0 / kappa, n) if n > 1 else np.ones(1)


def lam_cert_edge(n, c=4.0):
    """Spectrum of trace 1, geomspace(1, 1e-3) with the last eigenvalue c TAU (tr A = 1): c = 4 is the worst Gram a
    certificate admits with a margin, c = 0.5 must be refused and c = 2 certified."""
    lam = np.geomspace(1.0, 1.0e-3, n)
    lam[-1] = 0.0
    lam /= lam.sum()
    lam[-1] = c * TAU
    return lam


def indefinite_at(n, k, seed):
    """B B^T / n + I with the entry (k, k) lowered so that the pivot of column k is -0.5 while every earlier pivot
    is >= ~1 (pivots of an SPD matrix are bounded below by its smallest eigenvalue, here >= 1)."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    A = B @ B.T / n + np.eye(n)
    A = (A + A.T) / 2
    _, _, piv = chol_ld(A)
    tr = np.tril(A).astype(LD).diagonal().sum()
    A[k, k] = np.float64(LD(A[k, k]) - piv[k] * tr - LD(0.5))
    return A


def blocked_chol_f64(A, nb):
    """Plain float64 emulation of the algorithm class the kernels use, on the symmetric A: every nb x nb diagonal block
    is factored, inverted explicitly, the panel formed by multiplying with that inverse, and the trailing matrix
    updated. Returns (L, Z = L^{-1} by block forward substitution on the same block inverses)."""
    W = np.array(A, dtype=np.float64)
    n = W.shape[0]
    L = np.zeros((n, n))
    D = []
    for j0 in range(0, n, nb):
        j1 = min(j0 + nb, n)
        Ljj = np.linalg.cholesky(W[j0:j1, j0:j1])
        Zjj = np.linalg.inv(Ljj)
        D.append(Zjj)
        L[j0:j1, j0:j1] = Ljj
        if j1 < n:
            P = W[j1:, j0:j1] @ Zjj.T
            L[j1:, j0:j1] = P
            W[j1:, j1:] -= P @ P.T
    Z = np.zeros((n, n))
    for b, j0 in enumerate(range(0, n, nb)):
        j1 = min(j0 + nb, n)
        Z[j0:j1, j0:j1] = D[b]
        if j0:
            Z[j0:j1, :j0] = -D[b] @ (L[j0:j1, :j0] @ Z[:j0, :j0])
    return L, Z


def _fro(x):
    return np.sqrt((np.asarray(x, dtype=LD) ** 2).sum())


def _fro_sym(x):
    """Frobenius norm of a symmetric matrix from its lower triangle."""
    x = np.asarray(x, dtype=LD)
    return np.sqrt(2 * (np.tril(x, -1) ** 2).sum() + (x.diagonal() ** 2).sum())


def res_L(As, L):
    """||A_s - L L^T||_F / ||A_s||_F (L lower triangular, A_s symmetric)."""
    L = np.asarray(L, dtype=LD)
    return float(_fro_sym(As - tmm(L, L.T, x_lower=True, y_upper=True, lower_only=True)) / _fro_sym(As))


def res_Z(Z, L):
    """||Z L - I||_F / (||Z||_F ||L||_F) (Z, L and so Z L lower triangular)."""
    n = L.shape[0]
    return float(_fro(tmm(Z, L, x_lower=True, y_lower=True, lower_only=True) - np.eye(n, dtype=LD)) / (_fro(Z) * _fro(L)))


def white(As, Z):
    """max |Z A_s Z^T - I| (Z lower triangular, A_s symmetric)."""
    n = Z.shape[0]
    ZA = tmm(Z, As, x_lower=True)
    return float(np.abs(np.tril(tmm(ZA, np.asarray(Z, dtype=LD).T, y_upper=True, lower_only=True) - np.eye(n, dtype=LD))).max())


def factor_err(L, Lref):
    """||L - L_ref||_F / ||L_ref||_F."""
    return float(_fro(np.asarray(L, dtype=LD) - Lref) / _fro(Lref))


def forward_ld(L, Y):
    """L^{-1} Y by forward substitution in long double (L float64 lower triangular, Y n x m)."""
    L, X = np.asarray(L, dtype=LD), np.array(Y, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - np.dot(L[i, :i], X[:i])) / L[i, i]
    return X


# ------------------------------------------------------------------------------------------------- the tests' cases
# Orders, the smallest at which each mechanism can still go wrong: one tile, the tile edges, tile ownership wrapping
# over the 8 waves, all 17 slots in use; the 2 x 2 blocks with n2 = 1, n2 across a tile edge, full size; chol_full with
# a last block of 1, three blocks exactly, a fourth block of 1; the 32-wide kernel (mode 2, xrs_potrf_solve).
ORDERS_RR = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 128, 129, 240, 241, 255, 256)
ORDERS_2X2 = (257, 258, 272, 273, 300, 384, 511, 512)
ORDERS_FULL = (513, 520, 768, 769)
ORDERS_32 = (257, 288, 289, 320, 500, 512)
ORDERS_GRADED = (17, 100, 256, 300, 520)
SHIFTS = (0.0, 1.0e-9, -1.0e-11)
SCALE_EXP = 400


def well(n):
    """The well-conditioned matrix of an order (kappa = 100) and its spectrum."""
    lam = graded(n, 100.0)
    return spd(n, lam, 1000 + n), lam


def graded_cases(n):
    """(name, A, lam) of the graded matrices of an order: kappa 1e4, 1e8 and lambda_min = 4 TAU tr A."""
    out = []
    for name, lam in (("k1e4", graded(n, 1.0e4)), ("k1e8", graded(n, 1.0e8)), ("edge", lam_cert_edge(n, 4.0))):
        out.append((name, spd(n, lam, 2000 + n), lam))
    return out


def accuracy_jobs(n):
    """(shift, binary exponent of the scale of A) of the well-conditioned accuracy jobs of an order: every shift and
    both scales; above 256, where a long-double residual costs seconds, in three jobs instead of five."""
    if n <= 256:
        return [(0.0, 0), (1.0e-9, 0), (-1.0e-11, 0), (0.0, SCALE_EXP), (0.0, -SCALE_EXP)]
    return [(0.0, SCALE_EXP), (1.0e-9, 0), (-1.0e-11, -SCALE_EXP)]


GRADED_JOBS = (("k1e4", 0.0), ("k1e4", 1.0e-9), ("k1e8", 0.0), ("edge", 0.0), ("edge", -1.0e-11))


def kappa_shifted(lam, shift_rel):
    s = shift_rel * float(np.sum(lam))
    return float((np.max(lam) + s) / (np.min(lam) + s))


STATUS_ORDERS = (17, 100, 256, 300, 520)


def status_columns(n):
    """First, a middle and the last column; for the block paths also both sides of column 256."""
    ks = {0, n // 2, n - 1}
    if n > 256:
        ks |= {255, 256, 257}
    return sorted(ks)


CERT_ORDERS = (16, 17, 100, 250, 256, 300, 512, 600)


@functools.lru_cache(maxsize=None)
def _cert_seed(n):
    # |last pivot| = |lambda_min - TAU tr A| / q^2 with q the last entry of the smallest eigenvector: the first seed
    # whose q is small enough for the reference to decide both cases with |pivot| / tr A >= 2e-10
    for t in range(64):
        seed = 3000 + n + 1000 * t
        ok = True
        for c in (0.5, 2.0):
            _, status, piv = chol_ld(spd(n, lam_cert_edge(n, c), seed), -TAU)
            last = piv[status - 1] if status else piv.min()
            ok = ok and abs(last) >= 2.0e-10 and (status != 0) == (c < 1.0)
        if ok:
            return seed
    raise AssertionError("no decisive certificate input found")


def cert_case(n, c):
    """A certificate input: trace 1, lambda_min = c TAU (c = 0.5 must fail, c = 2 must pass)."""
    return spd(n, lam_cert_edge(n, c), _cert_seed(n))


# Groups of cases that share a bar (8 x the worst reference value over the group, rounded up to a power of two;
# tools/chol_bars.py). The well-conditioned ones are banded by order, and a test caps the bar of its order n at 16 n u:
# a kernel that needs more at kappa = 100 is a finding, not a reason for a wider bar.
WELL_GROUPS = {
    "n1_2": (1, 2),
    "n15_17": (15, 16, 17),
    "n31_49": (31, 32, 33, 47, 48, 49),
    "n100_129": (100, 128, 129),
    "n240_256": (240, 241, 255, 256),
    "b2x2": ORDERS_2X2,
    "full": ORDERS_FULL,
    "k32": ORDERS_32,
}
# graded: (orders, block sizes of the emulation: the path's own, nested paths the worst of theirs)
GRADED_GROUPS = {
    "rr": ((17, 100, 256), (16,)),
    "b2x2": ((300,), (16, 256)),
    "full": ((520,), (16, 256)),
    "k32": ((300,), (32,)),
}
TRSM_ORDERS = (1, 16, 17, 100, 256, 257, 289, 512)
TRSM_NVEC = (1, 15, 16, 17, 40)
TRSM_GROUPS = {"n1_17": (1, 16, 17), "n100_256": (100, 256), "n257_512": (257, 289, 512)}


def well_group_of(n, k32=False):
    if k32:
        return "k32"
    return next(g for g, orders in WELL_GROUPS.items() if g != "k32" and n in orders)


def rhs(n):
    """The right-hand sides of the triangular-solve tests: n x 40, the first nvec columns used."""
    return np.random.default_rng(5000 + n).standard_normal((n, max(TRSM_NVEC)))
