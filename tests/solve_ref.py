"""CPU reference of the dense solves (csrc/solve.hip: xrs_solve, xrs_solve_least_squares): the cases of
tests/test_solve_gpu.py, a numpy restatement of the reference's dispatch (is_symmetric / pos_neg_definite_diagonal,
blasLapackWrapper.cpp:501-538) that says which route each input must take, and a solution of every case that is far
more accurate than float64 LAPACK:

  exact    A and X0 have small integer or dyadic entries, B = A X0 is exact in float64 and the solution is X0;
  mp       every system with max(m, n) <= 64 (and every rank-deficient one, from its exact full-rank factors
           A = C F): mpmath at 40 digits, x = F^T (F F^T)^-1 (C^T C)^-1 C^T b, the minimum-norm least-squares solution;
  refined  LAPACK's solution refined with residuals accumulated in long double (64-bit mantissa, u_ld = 5.4e-20)
           by chol_ref.tmm: LU for square systems, the augmented system r + A x = b, A^T r = 0 (Bjorck) on a QR
           factorisation for least squares, and the same system on A^T for the minimum-norm solution of a wide one.

The bar of a case is 4 max(e_LAPACK, 16 u K): e_LAPACK the error of cho_solve / numpy.linalg.solve / lstsq(rcond = 8 eps)
on the same input, K the first-order condition of the problem (kappa_2 of A, of its kept part for a deficient system;
kappa + kappa^2 |r| / (|A| |x|) for least squares with residual r). Errors are |X - X_ref|_F / |X_ref|_F in long double.
tests/test_solve_ref_cpu.py proves that each reference is 100 times more accurate than the bar it is used for."""
import dataclasses
import functools

import mpmath
import numpy as np
import scipy.linalg as sla

import chol_ref as cr

LD = np.longdouble
U = 2.0 ** -53             # unit roundoff of float64
EPS = 2.0 ** -52           # DBL_EPSILON
RCOND = 8 * EPS            # the rank cut of k_inv_cut (dgelsd's rcond = xerus::EPSILON)
SMALL_MAX = 512            # min(m, n) above: the CholeskyQR3 QR / LQ route instead of the SVD
MP_MAX = 64                # max(m, n) up to which the reference is mpmath's
MP_DIGITS = 40


def fro(x):
    return np.sqrt((np.asarray(x, dtype=LD) ** 2).sum())


def err(X, Xref):
    """|X - X_ref|_F / |X_ref|_F in long double (X_ref = 0: 0 if X is exactly 0, else inf)."""
    X, Xref = np.asarray(X, dtype=LD).reshape(np.shape(Xref)), np.asarray(Xref, dtype=LD)
    nr = fro(Xref)
    if nr == 0:
        return 0.0 if not np.any(X) else float("inf")
    return float(fro(X - Xref) / nr)


# ------------------------------------------------------------------------------------------- the reference's dispatch
def ref_is_symmetric(A):
    """is_symmetric (:501-516): no pair with |A_ij - A_ji| >= 4 max(0, max A) eps. Returns (symmetric, threshold,
    largest asymmetry)."""
    A = np.asarray(A, dtype=np.float64)
    thr = 4 * max(0.0, float(A.max())) * EPS
    iu = np.triu_indices(A.shape[0], 1)
    d = np.abs(A[iu] - A.T[iu])
    return (not np.any(d >= thr)), thr, (float(d.max()) if d.size else 0.0)


def ref_posneg_diagonal(A):
    """pos_neg_definite_diagonal (:519-538): 'pos' (A_00 > 0, every other A_ii >= eps), 'neg' (A_00 <= 0, every other
    A_ii <= -eps) or None. The reference tries Cholesky on both; the kernel only on 'pos' (Cholesky of a matrix with a
    negative diagonal can only fail, and the general route follows either way)."""
    d = np.asarray(A, dtype=np.float64).diagonal()
    if d[0] > 0:
        return "pos" if np.all(d[1:] >= EPS) else None
    return "neg" if np.all(d[1:] <= -EPS) else None


def expected_route(A, least_squares=False):
    """The route of csrc/solve.hip for this input, from the restated dispatch and LAPACK's Cholesky alone."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    general = "svd" if min(m, n) <= SMALL_MAX else "qr"
    if least_squares or m != n or not ref_is_symmetric(A)[0] or ref_posneg_diagonal(A) != "pos":
        return general
    try:
        sla.cholesky(A, lower=True)
    except np.linalg.LinAlgError:
        return "cholesky_failed_" + general
    return "cholesky"


# --------------------------------------------------------------------------------------------------------- references
def _mp_to_ld(vals, shape):
    out = np.empty(int(np.prod(shape)), dtype=LD)
    for i, v in enumerate(vals):
        hi = float(v)
        out[i] = LD(hi) + LD(float(v - hi))
    return out.reshape(shape)


def _mp_solve(M, Y):
    """M^-1 Y for mpmath matrices (one LU, a pair of triangular solves per column)."""
    ctx = mpmath.mp
    LU, piv = ctx.LU_decomp(M)
    out = ctx.matrix(Y.rows, Y.cols)
    for j in range(Y.cols):
        x = ctx.U_solve(LU, ctx.L_solve(LU, Y[:, j], piv))
        for i in range(Y.rows):
            out[i, j] = x[i]
    return out


def mp_min_norm(C, F, B):
    """The minimum-norm least-squares solution of (C F) X = B at 40 digits, as long double: C (m x r) of full column
    rank, F (r x n) of full row rank, None standing for the identity (a square nonsingular A: C = A, F = None)."""
    B = np.asarray(B, dtype=np.float64)
    B2 = B.reshape(B.shape[0], -1)
    ctx = mpmath.mp
    with ctx.workdps(MP_DIGITS):
        Y = ctx.matrix(B2.tolist())
        if C is not None:
            Cm = ctx.matrix(np.asarray(C, dtype=np.float64).tolist())
            Y = _mp_solve(Cm, Y) if Cm.rows == Cm.cols else _mp_solve(Cm.T * Cm, Cm.T * Y)
        if F is not None:
            Fm = ctx.matrix(np.asarray(F, dtype=np.float64).tolist())
            Y = Fm.T * _mp_solve(Fm * Fm.T, Y)
        rows = Y.rows
        vals = [Y[i, j] for i in range(rows) for j in range(Y.cols)]
        return _mp_to_ld(vals, (rows,) + B.shape[1:])


def refine_square(A, B, steps=4):
    """A^-1 B for nonsingular A: LU, then `steps` corrections from long-double residuals. Returns (X in long double,
    |last correction|_F / |X|_F); each step gains a factor of about kappa n u."""
    A = np.asarray(A, dtype=np.float64)
    B2 = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1)
    lu = sla.lu_factor(A)
    X = sla.lu_solve(lu, B2).astype(LD)
    last = np.inf
    for _ in range(steps):
        R = B2.astype(LD) - cr.tmm(A, X)
        D = sla.lu_solve(lu, R.astype(np.float64))
        X = X + D.astype(LD)
        last = float(fro(D) / fro(X))
    return X.reshape((A.shape[1],) + np.shape(B)[1:]), last


def refine_augmented(T, f, g, steps=5):
    """(r, z) with r + T z = f and T^T r = g for a tall T (M x N) of full column rank, on T = Q R with residuals in
    long double. f = b, g = 0: z is the least-squares solution of T z = b and r its residual; f = 0, g = b: r is the
    minimum-norm solution of T^T r = b. Returns (r, z, |last correction| / |solution| over both)."""
    T = np.asarray(T, dtype=np.float64)
    Q, R = np.linalg.qr(T)
    f, g = np.asarray(f, dtype=LD), np.asarray(g, dtype=LD)
    r, z = np.zeros(f.shape, dtype=LD), np.zeros(g.shape, dtype=LD)
    last = np.inf
    for _ in range(steps + 1):   # (the first pass from zero is the plain QR solution)
        Fr = (f - r - cr.tmm(T, z)).astype(np.float64)
        Gr = (g - cr.tmm(T.T, r)).astype(np.float64)
        u = sla.solve_triangular(R, Gr, trans="T")
        qf = Q.T @ Fr
        dz = sla.solve_triangular(R, qf - u)
        dr = Q @ u + Fr - Q @ qf
        r, z = r + dr.astype(LD), z + dz.astype(LD)
        last = float(max(fro(dr) / max(fro(r), fro(f), LD(1e-300)), fro(dz) / max(fro(z), LD(1e-300))))
    return r, z, last


def refined(A, B):
    """The refined reference of a full-rank system of any shape: (X in long double, last relative correction)."""
    A = np.asarray(A, dtype=np.float64)
    B2 = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1)
    m, n = A.shape
    if m == n:
        X, last = refine_square(A, B2)
    elif m > n:
        _, X, last = refine_augmented(A, B2, np.zeros((n, B2.shape[1])))
    else:
        X, _, last = refine_augmented(A.T, np.zeros((n, B2.shape[1])), B2)
    return X.reshape((n,) + np.shape(B)[1:]), last


# -------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass
class Case:
    name: str
    group: str
    A: np.ndarray
    B: np.ndarray
    route: str                     # the route the GPU must report
    lapack: str                    # 'chol' | 'gesv' | 'gelsd': the LAPACK solver e_LAPACK comes from
    ref_kind: str                  # 'exact' | 'mp' | 'refined'
    xref: np.ndarray               # long double
    rank: int                      # intended numerical rank under rcond = 8 eps
    kappa: float = None            # intended kappa_2 (of the kept part), where the generator prescribes one
    least_squares: bool = False    # through xrs_solve_least_squares
    last_correction: float = 0.0   # refined references: the size of the last correction
    factors: tuple = None          # (C, F) of a deficient case

    @functools.cached_property
    def sigma(self):
        return np.linalg.svd(self.A, compute_uv=False)

    @functools.cached_property
    def kappa_kept(self):
        s = self.sigma
        return float(s[0] / s[self.rank - 1]) if self.rank else 1.0

    @functools.cached_property
    def K(self):
        """First-order condition of the problem."""
        k = self.kappa_kept
        m, n = self.A.shape
        if m <= n or self.rank < min(m, n) or not self.rank:
            return k
        B2 = self.B.reshape(m, -1).astype(LD)
        r = B2 - cr.tmm(self.A, self.xref.reshape(n, -1))
        return k + k * k * float(fro(r) / (LD(self.sigma[0]) * fro(self.xref)))

    @functools.cached_property
    def x_lapack(self):
        B2 = self.B.reshape(self.A.shape[0], -1)
        if self.lapack == "chol":
            X = sla.cho_solve(sla.cho_factor(self.A, lower=True), B2)
        elif self.lapack == "gesv":
            X = np.linalg.solve(self.A, B2)
        else:
            X = np.linalg.lstsq(self.A, B2, rcond=RCOND)[0]
        return X.reshape(self.xref.shape)

    @functools.cached_property
    def e_lapack(self):
        return err(self.x_lapack, self.xref)

    @functools.cached_property
    def bar(self):
        return 4 * max(self.e_lapack, 16 * U * self.K)


def spd64(n, kappa, seed):
    """Q diag(lam) Q^T in float64, symmetrised exactly, lam geometric from 1 to 1 / kappa: the eigenvalues are lam up to
    an absolute n u, which the CPU test pins through kappa."""
    Q = cr._orth(n, seed)
    A = (Q * cr.graded(n, kappa)) @ Q.T
    return (A + A.T) / 2


def general64(m, n, kappa, seed):
    """U diag(s) V^T with a geometric spectrum from 1 to 1 / kappa (nonsymmetric, full rank)."""
    k = min(m, n)
    rng = np.random.default_rng(seed)
    Uq = np.linalg.qr(rng.standard_normal((m, k)))[0]
    Vq = np.linalg.qr(rng.standard_normal((n, k)))[0]
    return (Uq * cr.graded(k, kappa)) @ Vq.T


def _rhs(A, p, seed, one_d=False):
    """(X0, B = A X0 rounded): a consistent right-hand side with Gaussian X0."""
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal((A.shape[1],) if one_d else (A.shape[1], p))
    return X0, A @ X0


def _make(name, group, A, B, lapack, ref_kind=None, xref=None, rank=None, kappa=None, least_squares=False, factors=None):
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    m, n = A.shape
    last = 0.0
    if xref is None:
        if factors is not None:
            ref_kind, xref = "mp", mp_min_norm(factors[0], factors[1], B)
        elif max(m, n) <= MP_MAX:
            ref_kind = "mp"
            xref = mp_min_norm(A if m >= n else None, A if m < n else None, B)
        else:
            ref_kind = "refined"
            xref, last = refined(A, B)
    return Case(name, group, A, B, expected_route(A, least_squares), lapack, ref_kind, np.asarray(xref, dtype=LD),
                min(m, n) if rank is None else rank, kappa, least_squares, last, factors)


# ---- Cholesky, block edges (kCholBlock = 256): every order with one p, every p at 257 and 513; a well-conditioned family
# (kappa = 100, as chol_ref.well) and a moderately conditioned one (kappa = 1e6)
CHOL_WELL = ((1, 1), (2, 3), (255, 3), (256, 65), (257, 1), (257, 3), (257, 65), (511, 1), (512, 3), (513, 1), (513, 3),
             (513, 65), (769, 65))
CHOL_MODERATE = ((2, 1), (255, 1), (256, 3), (257, 3), (511, 3), (512, 1), (513, 3), (769, 3))
KAPPA_WELL, KAPPA_MODERATE = 100.0, 1.0e6


def _chol_case(n, p, kappa, tag):
    A = spd64(n, kappa if n > 1 else 1.0, 7000 + n)
    _, B = _rhs(A, p, 7100 + n + p)
    return _make(f"chol_{tag}_n{n}_p{p}", "cholesky", A, B, "chol", kappa=kappa if n > 1 else 1.0)


# ---- fallback: symmetric, positive diagonal, first non-positive pivot at column k (k in the third 256-block at n = 600)
FALLBACK = ((40, 20), (300, 280), (600, 550))


def indefinite_posdiag(n, k, seed):
    """G G^T / n + I with the entry (k, k) halved towards l_k . l_k / 2, l_k the row of the Cholesky factor: the pivot
    of column k becomes -l_k . l_k / 2 < 0, the diagonal stays positive and every earlier pivot is untouched (>= 1)."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    A = G @ G.T / n + np.eye(n)
    A = (A + A.T) / 2
    Lk = np.linalg.cholesky(A[:k, :k])
    l = sla.solve_triangular(Lk, A[:k, k], lower=True)
    A[k, k] = 0.5 * float(l @ l)
    return A


def _fallback_case(n, k):
    A = indefinite_posdiag(n, k, 7200 + n)
    _, B = _rhs(A, 3, 7300 + n)
    return _make(f"fallback_n{n}_k{k}", "fallback", A, B, "gesv")


# ---- dispatch thresholds at n = 48
DISPATCH = ("asym_2eps", "asym_8eps", "diag_half_eps", "a00_zero", "negated", "no_positive_entry")
DISPATCH_N, DISPATCH_PAIR, DISPATCH_DIAG = 48, (3, 17), 5


def dispatch_matrix(kind):
    n = DISPATCH_N
    A = spd64(n, KAPPA_WELL, 7400)
    i, j = DISPATCH_PAIR
    if kind in ("asym_2eps", "asym_8eps"):
        A[i, j] += (2 if kind == "asym_2eps" else 8) * A.max() * EPS   # (the upper entry only)
    elif kind == "diag_half_eps":
        A[DISPATCH_DIAG, DISPATCH_DIAG] = EPS / 2
    elif kind == "a00_zero":
        A[0, 0] = 0.0
    elif kind == "negated":
        A = -A
    elif kind == "no_positive_entry":
        E = np.random.default_rng(7401).uniform(0.25, 1.0, (n, n))
        A = -((E + E.T) / 2 + n * np.eye(n))
    return A


def _dispatch_case(kind):
    A = dispatch_matrix(kind)
    _, B = _rhs(A, 3, 7410)
    return _make(f"dispatch_{kind}", "dispatch", A, B, "chol" if kind == "asym_2eps" else "gesv")


# ---- rank cut: A = C F exactly, C (m x r) and F (r x n) of small integers with duplicated and zero rows / columns;
# 'gap': the columns of C scaled by powers of two down to 2^-GAP_EXP, so the kept singular values spread over several
# orders of magnitude and the others stay exactly zero
RANKCUT = (("square", 24, 24, 17), ("tall", 60, 30, 11), ("wide", 30, 60, 11))
GAP_EXP = 14


def _int_full_rank(rows, r, rng):
    while True:
        M = rng.integers(-3, 4, (rows, r)).astype(np.float64)
        if np.linalg.matrix_rank(M) == r:
            return M


def deficient_factors(m, n, r, seed, gap=False):
    """(C, F): C has m - 4 distinct rows, two of them repeated, and two zero rows; F the same by columns."""
    rng = np.random.default_rng(seed)

    def tall(rows):
        base = _int_full_rank(rows - 4, r, rng)
        M = np.vstack([base, base[[1, 3]], np.zeros((2, r))])
        return M[rng.permutation(rows)]

    C, F = tall(m), tall(n).T
    if gap:
        C = C * np.ldexp(1.0, -np.round(np.linspace(0, GAP_EXP, r)).astype(int))[None, :]
    return C, F


def _rankcut_case(shape, m, n, r, gap, ls):
    C, F = deficient_factors(m, n, r, 7500 + m + n, gap)
    A = C @ F                                                        # exact: integers times powers of two
    X0 = np.random.default_rng(7600 + m).integers(-4, 5, (n, 3)).astype(np.float64)
    B = A @ X0                                                       # exact
    name = f"rankcut_{shape}{'_gap' if gap else ''}{'_ls' if ls else ''}"
    return _make(name, "rankcut", A, B, "gelsd", rank=r, least_squares=ls, factors=(C, F))


ZERO_SHAPES = ((24, 24), (60, 30), (30, 60))


def _zero_case(m, n):
    B = np.random.default_rng(7700).standard_normal((m, 3))
    return _make(f"zero_{m}x{n}", "rankcut", np.zeros((m, n)), B, "gelsd", ref_kind="exact", xref=np.zeros((n, 3)), rank=0)


# ---- the 512 | 513 boundary between the SVD and the CholeskyQR3 route: Gaussian, and kappa = 1e6 at (513, 513), (700, 513)
BOUNDARY = ((512, 512), (513, 513), (700, 512), (700, 513), (512, 700), (513, 700))
BOUNDARY_ILL = ((513, 513), (700, 513))
KAPPA_ILL = 1.0e6


def _boundary_case(m, n, ill):
    if ill:
        A = general64(m, n, KAPPA_ILL, 7800 + m + n)
        _, B = _rhs(A, 3, 7810 + m)          # consistent up to rounding: K = kappa, not kappa^2
    else:
        rng = np.random.default_rng(7820 + 3 * m + n)
        A, B = rng.standard_normal((m, n)), rng.standard_normal((m, 3))
    return _make(f"boundary_{m}x{n}{'_k1e6' if ill else ''}", "boundary", A, B, "gesv" if m == n else "gelsd",
                 kappa=KAPPA_ILL if ill else None)


# ---- refusal: min(m, n) > 512 with an exactly duplicated column, and the well-posed system that follows
REFUSAL = ((600, 600), (700, 560))


def refusal_matrix(m, n):
    A = np.random.default_rng(7900 + m).standard_normal((m, n))
    A[:, n - 7] = A[:, 11]
    return A


def _after_refusal_case(m, n):
    rng = np.random.default_rng(7910 + m)
    return _make(f"after_refusal_{m}x{n}", "refusal", rng.standard_normal((m, n)), rng.standard_normal((m, 3)),
                 "gesv" if m == n else "gelsd")


# ---- degenerate shapes, exact: small integers, B = A X0 (1-D B, and p = 1 through a 2-D B)
def _degenerate_cases():
    out = []
    out.append(_make("degenerate_1x1", "degenerate", [[4.0]], [2.0], "chol", ref_kind="exact", xref=[0.5]))
    out.append(_make("degenerate_1x1_negative", "degenerate", [[-4.0]], [[2.0]], "gesv", ref_kind="exact", xref=[[-0.5]]))
    out.append(_make("degenerate_1x5", "degenerate", [[1.0, -2.0, 0.0, 3.0, 1.0]], [[6.0]], "gelsd"))
    out.append(_make("degenerate_1x5_1d", "degenerate", [[1.0, -2.0, 0.0, 3.0, 1.0]], [6.0], "gelsd"))
    a51 = [[2.0], [-1.0], [0.0], [3.0], [1.0]]
    out.append(_make("degenerate_5x1", "degenerate", a51, [[1.0], [2.0], [-3.0], [0.0], [5.0]], "gelsd"))
    out.append(_make("degenerate_5x1_1d", "degenerate", a51, [1.0, 2.0, -3.0, 0.0, 5.0], "gelsd"))
    rng = np.random.default_rng(8000)
    M = rng.integers(-2, 3, (7, 7)).astype(np.float64)
    S = M @ M.T + 7 * np.eye(7)                         # SPD, integers
    N = M + 5 * np.eye(7)                               # nonsymmetric, nonsingular (pinned by the CPU test)
    x1 = rng.integers(-4, 5, 7).astype(np.float64)
    for tag, A, lapack in (("spd", S, "chol"), ("general", N, "gesv")):
        out.append(_make(f"degenerate_7x7_{tag}_1d", "degenerate", A, A @ x1, lapack, ref_kind="exact", xref=x1))
        out.append(_make(f"degenerate_7x7_{tag}_p1", "degenerate", A, (A @ x1)[:, None], lapack, ref_kind="exact",
                         xref=x1[:, None]))
    return out


_BUILDERS = {}
for _n, _p in CHOL_WELL:
    _BUILDERS[f"chol_well_n{_n}_p{_p}"] = functools.partial(_chol_case, _n, _p, KAPPA_WELL, "well")
for _n, _p in CHOL_MODERATE:
    _BUILDERS[f"chol_moderate_n{_n}_p{_p}"] = functools.partial(_chol_case, _n, _p, KAPPA_MODERATE, "moderate")
for _n, _k in FALLBACK:
    _BUILDERS[f"fallback_n{_n}_k{_k}"] = functools.partial(_fallback_case, _n, _k)
for _kind in DISPATCH:
    _BUILDERS[f"dispatch_{_kind}"] = functools.partial(_dispatch_case, _kind)
for _shape, _m, _n, _r in RANKCUT:
    for _gap in (False, True):
        for _ls in (False, True):
            _BUILDERS[f"rankcut_{_shape}{'_gap' if _gap else ''}{'_ls' if _ls else ''}"] = functools.partial(
                _rankcut_case, _shape, _m, _n, _r, _gap, _ls)
for _m, _n in ZERO_SHAPES:
    _BUILDERS[f"zero_{_m}x{_n}"] = functools.partial(_zero_case, _m, _n)
for _m, _n in BOUNDARY:
    _BUILDERS[f"boundary_{_m}x{_n}"] = functools.partial(_boundary_case, _m, _n, False)
for _m, _n in BOUNDARY_ILL:
    _BUILDERS[f"boundary_{_m}x{_n}_k1e6"] = functools.partial(_boundary_case, _m, _n, True)
for _m, _n in REFUSAL:
    _BUILDERS[f"after_refusal_{_m}x{_n}"] = functools.partial(_after_refusal_case, _m, _n)
DEGENERATE = ("degenerate_1x1", "degenerate_1x1_negative", "degenerate_1x5", "degenerate_1x5_1d", "degenerate_5x1",
              "degenerate_5x1_1d", "degenerate_7x7_spd_1d", "degenerate_7x7_spd_p1", "degenerate_7x7_general_1d",
              "degenerate_7x7_general_p1")


@functools.lru_cache(maxsize=None)
def _degenerate_table():
    return {c.name: c for c in _degenerate_cases()}


for _name in DEGENERATE:
    _BUILDERS[_name] = functools.partial(lambda nm: _degenerate_table()[nm], _name)


def names(prefix=""):
    return [k for k in _BUILDERS if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of a name: built once, shared by the tests that use it, never modified."""
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    for a in (c.A, c.B, c.xref):
        a.setflags(write=False)
    return c
