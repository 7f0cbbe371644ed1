"""xrs_solve / xrs_solve_least_squares (csrc/solve.hip) through Handle.solve: every case asserts the route the call
took (Handle.solve_last_path) and the result against the high-precision reference of tests/solve_ref.py.

The fallback from the blocked Cholesky to the SVD / CholeskyQR3 solve is as accurate as Cholesky on a well-conditioned
SPD system, so a result alone cannot tell a Cholesky that always refuses from one that works: the route can. The groups:
the Cholesky block edges (kCholBlock = 256: orders 1 .. 769, right-hand sides 1, 3, 65 wide), Cholesky refused in the
first, second and third diagonal block, the thresholds of the dispatch (k_sym_flags), the rank cut of the pseudo-inverse
(k_inv_cut) against the minimum-norm solution, the min(m, n) = 512 | 513 boundary between the SVD and the QR / LQ
route, the documented refusal of the latter, and the degenerate shapes.

The bar of a case is 4 max(e_LAPACK, 16 u K) (solve_ref.Case.bar); tests/test_solve_ref_cpu.py pins every input and
proves the references. Each test prints the measured error and the bar.

Largest error / bar per group on the MI355X: cholesky 0.0068 (kappa = 100: errors 3.5e-15 .. 4.8e-15 against LAPACK's
4e-15 .. 6e-15; kappa = 1e6: 1.7e-11 .. 2.9e-11 against 2e-11 .. 3.5e-11), fallback 0.0048, dispatch 0.0105, rank cut 0.0100
(norm excess at most 3.6e-14), boundary 0.0092 (kappa = 1e6 through CholeskyQR3: 6.5e-11 and 4.7e-11 against LAPACK's
4.1e-11 and 2.7e-11), after a refusal 0.0023, degenerate 0.0084. Every route was the expected one.

What the tests found: the 700 x 560 system with a duplicated column was not refused. The second Cholesky pass of the
CholeskyQR3 route met a rounding-size positive pivot, all three factorisations reported success and the call returned a
solution of norm 3e14 (dgelsd: 3.3) with status 0; 600 x 600 was refused only because its noise pivot came out negative.
qr_solve_big now refuses a second-pass pivot below 16 (m + n) u (k_pivot_floor).
"""
import numpy as np
import pytest

import solve_ref as sr

pytestmark = pytest.mark.gpu

XRS_ENUMERIC = 1


def _solve(handle, A, B, least_squares=False):
    dA, dB = handle.array(A), handle.array(B)
    dX = handle.solve(dA, dB, least_squares=least_squares)
    X, route = dX.numpy(), handle.solve_last_path()
    for d in (dA, dB, dX):
        d.free()
    return X, route


def _check(handle, name, route):
    """Route and result of one case; returns (X, case)."""
    c = sr.case(name)
    assert c.route == route           # (the restated dispatch agrees with what the test is for)
    X, got = _solve(handle, c.A, c.B, c.least_squares)
    e = sr.err(X, c.xref)
    print(f"solve {name}: route {got}, error {e:.2e}, bar {c.bar:.2e} (LAPACK {c.e_lapack:.2e}, K {c.K:.2e}), ratio {e / c.bar:.3f}")
    assert got == route
    assert X.shape == c.xref.shape
    assert e <= c.bar
    return X, c


@pytest.mark.parametrize("name", sr.names("chol_"))
def test_cholesky_block_edges(handle, name):
    """SPD at both sides of every 256-block edge, odd orders (odd leading dimension: every panel view off the 16-byte
    alignment), a last block of one row, ragged right-hand sides: Cholesky, never 'attempted and failed'."""
    _check(handle, name, "cholesky")


@pytest.mark.parametrize("name", sr.names("fallback_"))
def test_cholesky_refused_falls_back(handle, name):
    """Symmetric, positive diagonal, indefinite, the first non-positive pivot in block 0, 1 and 2: Cholesky is tried,
    refuses, and the general route of the size solves the system."""
    n = sr.case(name).A.shape[0]
    _check(handle, name, "cholesky_failed_svd" if n <= sr.SMALL_MAX else "cholesky_failed_qr")


@pytest.mark.parametrize("name", sr.names("dispatch_"))
def test_dispatch_thresholds(handle, name):
    """An asymmetry of half and of twice the threshold 4 max(A) eps, a diagonal entry below eps at i = 5, A_00 = 0, an
    all-negative diagonal, no positive entry at all (threshold 0: every pair fails it)."""
    _check(handle, name, "cholesky" if name == "dispatch_asym_2eps" else "svd")


@pytest.mark.parametrize("name", sr.names("rankcut_"))
def test_rank_cut_minimum_norm(handle, name):
    """Exactly rank-deficient systems (duplicated and zero rows and columns), square, tall and wide, flat and with a
    spectrum spread down to the cut's neighbourhood but never near it: the minimum-norm solution, and a norm that does
    not exceed the minimum by more than the bar (the refinement steps must not leak into the null space)."""
    X, c = _check(handle, name, "svd")
    over = float(sr.fro(X) / sr.fro(c.xref)) - 1.0
    print(f"solve {name}: |X| / |X_ref| - 1 = {over:.2e}")
    assert over <= c.bar


@pytest.mark.parametrize("name", sr.names("zero_"))
@pytest.mark.parametrize("least_squares", [False, True])
def test_zero_matrix(handle, name, least_squares):
    """sigma_0 = 0: nothing passes S[i] > rcond S[0], X = 0 exactly."""
    c = sr.case(name)
    X, route = _solve(handle, c.A, c.B, least_squares)
    assert route == "svd"
    assert X.shape == c.xref.shape and np.array_equal(X, np.zeros(X.shape))


@pytest.mark.parametrize("name", sr.names("boundary_"))
def test_svd_qr_boundary(handle, name):
    """min(m, n) = 512: the SVD pseudo-inverse; 513: the CholeskyQR3 QR (square, tall) / LQ (wide) solve, also at
    kappa = 1e6."""
    c = sr.case(name)
    route = "svd" if min(c.A.shape) <= sr.SMALL_MAX else "qr"
    _check(handle, name, route)
    X, got = _solve(handle, c.A, c.B, least_squares=True)
    e = sr.err(X, c.xref)
    print(f"solve {name} (least squares entry): route {got}, error {e:.2e}, bar {c.bar:.2e}, ratio {e / c.bar:.3f}")
    assert got == route and e <= c.bar


def _refused(handle, dA, dB, least_squares):
    """The status of a solve that must be refused (None if it was not); keeps no reference to the exception."""
    from xerus_amd import capi

    try:
        handle.solve(dA, dB, least_squares=least_squares).free()
    except capi.XrsError as e:
        return e.code
    return None


@pytest.mark.parametrize("m,n", sr.REFUSAL)
def test_refusal_of_deficient_system_above_512(handle, m, n):
    """An exactly duplicated column with min(m, n) > 512: XRS_ENUMERIC from both entries, no pool block left behind by
    the refusal (a repeated refusal needs no new memory), and the next well-posed solve on the handle is right."""
    A = sr.refusal_matrix(m, n)
    B = np.random.default_rng(m + n).standard_normal((m, 3))
    dA, dB = handle.array(A), handle.array(B)
    held = []
    for least_squares in (False, True, False):
        assert _refused(handle, dA, dB, least_squares) == XRS_ENUMERIC
        assert handle.solve_last_path() == "qr"
        held.append(handle.pool_bytes())
    assert held[1] == held[0] and held[2] == held[0]
    dA.free()
    dB.free()
    _check(handle, f"after_refusal_{m}x{n}", "qr")


DEGENERATE_ROUTES = {
    "degenerate_1x1": "cholesky", "degenerate_1x1_negative": "svd",
    "degenerate_1x5": "svd", "degenerate_1x5_1d": "svd", "degenerate_5x1": "svd", "degenerate_5x1_1d": "svd",
    "degenerate_7x7_spd_1d": "cholesky", "degenerate_7x7_spd_p1": "cholesky",
    "degenerate_7x7_general_1d": "svd", "degenerate_7x7_general_p1": "svd",
}


@pytest.mark.parametrize("name", sr.DEGENERATE)
def test_degenerate_shapes(handle, name):
    """m or n = 1, a 1-D right-hand side, p = 1 through a 2-D one."""
    _check(handle, name, DEGENERATE_ROUTES[name])


def test_route_report_belongs_to_the_handle(handle):
    """A fresh handle reports no route, and a solve on it does not change another handle's report."""
    from xerus_amd import capi

    c = sr.case("degenerate_7x7_spd_p1")
    _, route = _solve(handle, c.A, c.B)
    assert route == "cholesky"
    h = capi.Handle(0)
    try:
        assert h.solve_last_path() is None
        g = sr.case("degenerate_7x7_general_p1")
        _, route = _solve(h, g.A, g.B)
        assert route == "svd" and h.solve_last_path() == "svd"
        assert handle.solve_last_path() == "cholesky"
    finally:
        h.close()
