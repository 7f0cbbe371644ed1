"""CPU: the reference of the dense-solve tests (tests/solve_ref.py) against mpmath, exact solutions and LAPACK, and the
proof that every input of tests/test_solve_gpu.py is what its name says: its numerical rank under rcond = 8 eps, its
kappa_2, the side of each dispatch threshold it falls on (a numpy restatement of the reference's is_symmetric /
pos_neg_definite_diagonal plus LAPACK's Cholesky), and that LAPACK's own solution meets the case's bar. So a failure
of the GPU test is never the input's fault. Every figure is printed (pytest -s)."""
import numpy as np
import pytest
import scipy.linalg as sla

import chol_ref as cr
import solve_ref as sr

FLOOR = 16 * sr.U          # bar = 4 max(e_LAPACK, FLOOR K); a reference must be 100 x better than the bar


def _floor_bar(K):
    return 4 * FLOOR * K


# ------------------------------------------------------------------------------- the reference tools are accurate enough
@pytest.mark.parametrize("m,n", [(40, 40), (64, 64), (60, 30), (30, 60), (5, 1), (1, 5)])
def test_refined_matches_mpmath(m, n):
    """The long-double-refined reference against mpmath at 40 digits on Gaussian systems (inconsistent where m > n):
    100 x below the smallest bar a case of this condition can have."""
    rng = np.random.default_rng(100 * m + n)
    A, B = rng.standard_normal((m, n)), rng.standard_normal((m, 3))
    X, last = sr.refined(A, B)
    Xmp = sr.mp_min_norm(A if m >= n else None, A if m < n else None, B)
    s = np.linalg.svd(A, compute_uv=False)
    e = sr.err(X, Xmp)
    print(f"refined vs mpmath {m}x{n}: {e:.2e} (kappa {s[0] / s[-1]:.1e}, last correction {last:.1e})")
    assert e <= _floor_bar(s[0] / s[-1]) / 100
    assert last <= _floor_bar(s[0] / s[-1]) / 100


@pytest.mark.parametrize("kappa", [1.0e2, 1.0e6])
def test_refined_matches_mpmath_conditioned(kappa):
    A = sr.general64(48, 48, kappa, 5)
    _, B = sr._rhs(A, 2, 6)
    X, _ = sr.refined(A, B)
    e = sr.err(X, sr.mp_min_norm(A, None, B))
    print(f"refined vs mpmath 48x48 kappa {kappa:.0e}: {e:.2e}")
    assert e <= _floor_bar(kappa) / 100
    T = sr.general64(60, 30, kappa, 7)
    _, B = sr._rhs(T, 2, 8)
    for M, C, F in ((T, T, None), (T.T.copy(), None, T.T.copy())):
        Bm = B if M is T else sr._rhs(M, 2, 9)[1]
        X, _ = sr.refined(M, Bm)
        e = sr.err(X, sr.mp_min_norm(C, F, Bm))
        print(f"refined vs mpmath {M.shape[0]}x{M.shape[1]} kappa {kappa:.0e}: {e:.2e}")
        assert e <= _floor_bar(kappa) / 100


def _exact_systems():
    rng = np.random.default_rng(42)
    M = rng.integers(-1, 2, (769, 769)).astype(np.float64)
    yield "spd 769", M @ M.T + 769 * np.eye(769), rng.integers(-4, 5, (769, 3)).astype(np.float64)
    n = 513
    yield "second difference 513", 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1), rng.integers(-4, 5, (n, 3)).astype(np.float64)
    yield "tall 700x513", rng.integers(-3, 4, (700, 513)).astype(np.float64), rng.integers(-4, 5, (513, 3)).astype(np.float64)
    yield "general 600", rng.integers(-3, 4, (600, 600)).astype(np.float64), rng.integers(-4, 5, (600, 3)).astype(np.float64)


def test_refined_recovers_exact_solutions():
    """Integer A and X0 at the sizes where mpmath is too slow: B = A X0 is exact, so the solution is X0."""
    for name, A, X0 in _exact_systems():
        B = A @ X0
        assert np.array_equal(cr.tmm(A, X0).astype(np.float64), B) and np.abs(B).max() < 2.0 ** 53
        X, last = sr.refined(A, B)
        s = np.linalg.svd(A, compute_uv=False)
        e = sr.err(X, X0)
        print(f"refined vs exact {name}: {e:.2e} (kappa {s[0] / s[-1]:.1e}, last correction {last:.1e})")
        assert e <= _floor_bar(s[0] / s[-1]) / 100


def test_mp_min_norm_of_exact_factors():
    """A = C F with integer factors: the mpmath solution is a least-squares solution (A^T (A x - b) = 0), lies in the
    row space (x = F^T w) and equals A^+ b of LAPACK to LAPACK's accuracy."""
    C, F = sr.deficient_factors(60, 30, 11, 1)
    A = C @ F
    B = np.random.default_rng(2).standard_normal((60, 2))        # inconsistent
    X = sr.mp_min_norm(C, F, B)
    g = cr.tmm(A.T, cr.tmm(A, X) - B.astype(sr.LD))
    s = np.linalg.svd(A, compute_uv=False)
    assert float(sr.fro(g)) <= 1e-16 * s[0] ** 2 * float(sr.fro(X))
    w = np.linalg.lstsq(F.T, X.astype(np.float64), rcond=None)[0]
    assert sr.err(F.T @ w, X) <= 1e-13
    assert sr.err(np.linalg.pinv(A, rcond=sr.RCOND) @ B, X) <= 1e-11


def test_err_measure():
    assert sr.err(np.zeros(3), np.zeros(3)) == 0.0
    assert sr.err(np.array([0.0, 1e-300, 0.0]), np.zeros(3)) == float("inf")
    assert sr.err(np.array([1.0, 1.0 + 2.0 ** -52]), np.array([1.0, 1.0])) == pytest.approx(2.0 ** -52 / np.sqrt(2))


def test_route_names_match_the_header():
    """capi.SOLVE_PATHS names exactly the values include/xerus_amd.h defines (XRS_SOLVE_CHOL_FAILED is a flag)."""
    import os
    import re

    from xerus_amd import capi

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xerus_amd.h")).read()
    v = {k: int(x) for k, x in re.findall(r"#define XRS_SOLVE_(\w+) (\d+)", hdr)}
    assert v == {"CHOLESKY": 1, "SVD": 2, "QR": 3, "CHOL_FAILED": 4}
    assert capi.SOLVE_PATHS == {0: None, v["CHOLESKY"]: "cholesky", v["SVD"]: "svd", v["QR"]: "qr",
                                v["CHOL_FAILED"] | v["SVD"]: "cholesky_failed_svd", v["CHOL_FAILED"] | v["QR"]: "cholesky_failed_qr"}
    assert capi.XRS_ENUMERIC == int(re.search(r"#define XRS_ENUMERIC (\d+)", hdr).group(1))


# --------------------------------------------------------------------------------------------- the restated dispatch
def test_restated_dispatch():
    A = np.array([[2.0, 1.0], [1.0, 3.0]])
    assert sr.ref_is_symmetric(A)[0] and sr.ref_posneg_diagonal(A) == "pos" and sr.expected_route(A) == "cholesky"
    assert sr.expected_route(A, least_squares=True) == "svd"
    assert sr.ref_posneg_diagonal(-A) == "neg" and sr.expected_route(-A) == "svd"
    A[0, 1] += 4 * 3.0 * sr.EPS          # exactly the threshold: >= makes it nonsymmetric
    assert not sr.ref_is_symmetric(A)[0] and sr.expected_route(A) == "svd"
    Z = np.array([[1.0, 2.0], [2.0, 1.0]])   # symmetric, positive diagonal, indefinite
    assert sr.expected_route(Z) == "cholesky_failed_svd"
    assert sr.ref_posneg_diagonal(np.diag([1.0, sr.EPS / 2])) is None
    assert sr.ref_posneg_diagonal(np.diag([1.0, sr.EPS])) == "pos"
    assert sr.ref_posneg_diagonal(np.diag([0.0, 1.0])) is None
    assert not sr.ref_is_symmetric(-np.ones((2, 2)))[0]        # max = 0: every pair fails 0 >= 0
    assert sr.expected_route(np.ones((513, 700))) == "qr" and sr.expected_route(np.ones((512, 700))) == "svd"


# ------------------------------------------------------------------------------------------------- every case's intent
INTENDED_ROUTE = {
    "chol_": "cholesky",
    "fallback_n40_k20": "cholesky_failed_svd", "fallback_n300_k280": "cholesky_failed_svd",
    "fallback_n600_k550": "cholesky_failed_qr",
    "dispatch_asym_2eps": "cholesky", "dispatch_": "svd",
    "rankcut_": "svd", "zero_": "svd",
    "boundary_512x512": "svd", "boundary_700x512": "svd", "boundary_512x700": "svd", "boundary_": "qr",
    "after_refusal_": "qr",
    "degenerate_1x1_negative": "svd", "degenerate_1x1": "cholesky", "degenerate_1x5": "svd", "degenerate_5x1": "svd",
    "degenerate_7x7_spd": "cholesky", "degenerate_7x7_general": "svd",
}


def intended_route(name):
    """Longest matching prefix of INTENDED_ROUTE."""
    return INTENDED_ROUTE[max((k for k in INTENDED_ROUTE if name.startswith(k)), key=len)]


@pytest.mark.parametrize("name", sr.names())
def test_case_intent(name):
    c = sr.case(name)
    m, n = c.A.shape
    # the rank under the kernel's cut, from LAPACK
    rank = int(np.linalg.lstsq(c.A, c.B.reshape(m, -1), rcond=sr.RCOND)[2]) if np.any(c.A) else 0
    s = c.sigma
    below = s[c.rank] / s[0] if c.rank < min(m, n) and s[0] > 0 else 0.0
    print(f"{name}: {m}x{n} rank {rank} kappa(kept) {c.kappa_kept:.3e} K {c.K:.3e} route {c.route} reference {c.ref_kind}"
          f" e_LAPACK {c.e_lapack:.2e} = {c.e_lapack / (FLOOR * c.K):.2f} x 16 u K, bar {c.bar:.2e}")
    assert rank == c.rank
    if c.rank:   # nothing near the cut: the kept values >= 1e-6 sigma_0 (up to the rounding of A), the others at rounding level
        assert s[c.rank - 1] / s[0] >= 0.99e-6 and below <= sr.RCOND / 4
    if c.kappa is not None:
        assert abs(c.kappa_kept / c.kappa - 1) <= 0.01
    # the dispatch: the restated reference rules give the route the generator is for
    assert c.route == intended_route(name)
    if c.route == "cholesky" and n > 1:
        assert np.linalg.eigvalsh((c.A + c.A.T) / 2)[0] > 0
    # the reference is 100 x better than the bar, LAPACK meets the bar and agrees with the reference to first order
    if c.ref_kind == "refined":
        assert c.last_correction <= c.bar / 100
    assert c.e_lapack <= c.bar
    assert c.e_lapack <= 100 * FLOOR * c.K
    assert c.xref.shape == (n,) + c.B.shape[1:]


def test_cholesky_orders_and_widths():
    """Every order of the issue with one p, every p at 257 and 513, in the well-conditioned family."""
    assert {n for n, _ in sr.CHOL_WELL} == {1, 2, 255, 256, 257, 511, 512, 513, 769}
    for n in (257, 513):
        assert {p for nn, p in sr.CHOL_WELL if nn == n} == {1, 3, 65}
    assert {p for _, p in sr.CHOL_WELL} == {1, 3, 65}


@pytest.mark.parametrize("n,k", sr.FALLBACK)
def test_fallback_inputs_are_decisive(n, k):
    """Exactly symmetric, diagonal well above eps, and the long-double Cholesky stops at column k with a pivot that
    rounding (about n u tr A) cannot move across zero; every earlier pivot is >= 0.5."""
    A = sr.case(f"fallback_n{n}_k{k}").A
    assert np.array_equal(A, A.T) and A.diagonal().min() >= 0.05
    assert sr.ref_is_symmetric(A)[0] and sr.ref_posneg_diagonal(A) == "pos"
    _, status, piv = cr.chol_ld(A)
    tr = float(np.trace(A))
    print(f"fallback n={n}: status {status}, pivot {float(piv[k]) * tr:.3f}, smallest earlier pivot {float(piv[:k].min()) * tr:.3f},"
          f" A[k][k] = {A[k, k]:.3f}")
    assert status == k + 1
    assert piv[k] * tr <= -0.05 and np.all(piv[:k] * tr >= 0.5)
    assert k // 256 == {40: 0, 300: 1, 600: 2}[n]
    with pytest.raises(np.linalg.LinAlgError):
        sla.cholesky(A, lower=True)


def test_dispatch_sides():
    """Which side of each threshold of is_symmetric / pos_neg_definite_diagonal the dispatch inputs fall on."""
    A0 = sr.dispatch_matrix("spd")
    assert sr.ref_is_symmetric(A0) == (True, 4 * A0.max() * sr.EPS, 0.0) and sr.ref_posneg_diagonal(A0) == "pos"
    i, j = sr.DISPATCH_PAIR
    for kind, lo, hi, sym in (("asym_2eps", 0.25, 0.75, True), ("asym_8eps", 1.75, 2.25, False)):
        A = sr.dispatch_matrix(kind)
        ok, thr, asym = sr.ref_is_symmetric(A)
        print(f"{kind}: asymmetry {asym:.3e} = {asym / thr:.3f} x threshold")
        assert ok == sym and lo * thr <= asym <= hi * thr and thr == 4 * A0.max() * sr.EPS
        assert abs(A[i, j] - A[j, i]) == asym and sr.ref_posneg_diagonal(A) == "pos"
    A = sr.dispatch_matrix("diag_half_eps")
    assert sr.ref_is_symmetric(A)[0] and sr.ref_posneg_diagonal(A) is None and A[0, 0] > 0
    assert A[sr.DISPATCH_DIAG, sr.DISPATCH_DIAG] == sr.EPS / 2 and sr.DISPATCH_DIAG > 0
    A = sr.dispatch_matrix("a00_zero")
    assert sr.ref_is_symmetric(A)[0] and A[0, 0] == 0 and np.all(A.diagonal()[1:] >= sr.EPS)
    assert sr.ref_posneg_diagonal(A) is None
    A = sr.dispatch_matrix("negated")
    assert sr.ref_is_symmetric(A)[0] and sr.ref_posneg_diagonal(A) == "neg" and np.array_equal(A, -A0)
    A = sr.dispatch_matrix("no_positive_entry")
    ok, thr, _ = sr.ref_is_symmetric(A)
    assert np.array_equal(A, A.T) and A.max() < 0 and thr == 0.0 and not ok


def test_deficient_inputs_are_exact():
    """A = C F and B = A X0 are exact in float64, A has exactly duplicated and zero rows and columns, and the
    spectrum of the 'gap' inputs spreads over at least three orders of magnitude."""
    for shape, m, n, r in sr.RANKCUT:
        for gap in (False, True):
            c = sr.case(f"rankcut_{shape}{'_gap' if gap else ''}")
            C, F = c.factors
            assert np.array_equal(cr.tmm(C, F).astype(np.float64), c.A) and np.array_equal(cr.tmm(C, F), c.A.astype(sr.LD))
            assert np.linalg.matrix_rank(C) == r and np.linalg.matrix_rank(F) == r and c.A.shape == (m, n)
            zr, zc = int(np.sum(~c.A.any(axis=1))), int(np.sum(~c.A.any(axis=0)))
            dr = m - len({row.tobytes() for row in c.A})
            dc = n - len({col.tobytes() for col in c.A.T})
            assert zr == 2 and zc == 2 and dr >= 3 and dc >= 3   # (the two zero rows count as one duplicate)
            assert float(sr.fro(cr.tmm(c.A, c.xref) - c.B.astype(sr.LD))) <= 1e-17 * c.sigma[0] * float(sr.fro(c.xref)) * c.kappa_kept
            if gap:
                assert c.kappa_kept >= 1e3
            print(f"rankcut_{shape}{'_gap' if gap else ''}: kappa of the kept part {c.kappa_kept:.2e}, "
                  f"sigma_r / sigma_0 = {c.sigma[r] / c.sigma[0]:.1e}")


@pytest.mark.parametrize("m,n", sr.REFUSAL)
def test_refusal_inputs(m, n):
    A = sr.refusal_matrix(m, n)
    assert min(m, n) > sr.SMALL_MAX and np.array_equal(A[:, n - 7], A[:, 11])
    s = np.linalg.svd(A, compute_uv=False)
    assert s[-1] / s[0] <= sr.RCOND / 4 and s[-2] / s[0] >= 1e-4
    assert sr.expected_route(A) == "qr"
