"""CPU: the reference of the batched Cholesky tests (tests/chol_ref.py) against LAPACK, and the proof that every status
and certificate input of tests/test_chol_batch_gpu.py is decisive: the long-double reference decides it with a margin
that float64 rounding (about n u = 1e-13 relative to tr A) cannot cross."""
import numpy as np
import pytest

import chol_ref as cr


@pytest.mark.parametrize("n", [1, 2, 17, 100, 300])
def test_chol_ld_matches_lapack(n):
    A, _ = cr.well(n)
    L, status, piv = cr.chol_ld(A)
    assert status == 0 and np.all(piv > 0)
    Lnp = np.linalg.cholesky(A)
    assert cr.factor_err(Lnp, L) <= 100 * n * cr.U   # kappa = 100: LAPACK's forward error
    assert np.array_equal(np.triu(L, 1), np.zeros((n, n)))
    assert cr.res_L(cr.shifted(A, 0.0), L) <= 1e-18
    # the shift is relative to the trace
    Ls, _, _ = cr.chol_ld(A, 1e-3)
    ref = np.linalg.cholesky(A + 1e-3 * np.trace(A) * np.eye(n))
    assert cr.factor_err(ref, Ls) <= 100 * n * cr.U


def test_chol_ld_reads_the_lower_triangle_only():
    A, _ = cr.well(40)
    B = A.copy()
    B[np.triu_indices(40, 1)] = np.nan
    L0, s0, p0 = cr.chol_ld(A)
    L1, s1, p1 = cr.chol_ld(B)
    assert s0 == s1 == 0 and np.array_equal(L0, L1) and np.array_equal(p0, p1)
    assert np.array_equal(cr.shifted(A, 1e-9), cr.shifted(B, 1e-9))


def test_pivot_rule():
    for bad in (2e300, 0.0, -1.0):
        A = np.eye(5) * 2.0
        A[3, 3] = bad
        assert cr.chol_ld(A)[1] == 4, bad
    for bad in (np.nan, np.inf):   # (the trace, and with it the shift of every diagonal entry, is not finite either)
        A = np.eye(5) * 2.0
        A[3, 3] = bad
        assert cr.chol_ld(A)[1] != 0, bad
    assert cr.chol_ld(np.zeros((6, 6)))[1] == 1


def test_blocked_emulation_is_a_cholesky():
    A, _ = cr.well(100)
    As = cr.shifted(A, 0.0)
    for nb in (16, 32, 256):
        L, Z = cr.blocked_chol_f64(A, nb)
        assert cr.res_L(As, L) <= 16 * 100 * cr.U
        assert cr.res_Z(Z, L) <= 16 * 100 * cr.U
        assert cr.white(As, Z) <= 100 * 16 * 100 * cr.U


def test_forward_substitution():
    A, _ = cr.well(33)
    L = np.linalg.cholesky(A)
    Y = np.random.default_rng(5).standard_normal((33, 4))
    X = cr.forward_ld(L, Y)
    assert np.abs(cr.mm(L, X) - Y).max() <= 1e-17


@pytest.mark.parametrize("n", cr.STATUS_ORDERS)
def test_status_inputs_are_decisive(n):
    """indefinite_at(n, k): the reference reports exactly k + 1, the failing pivot is <= -1e-3 tr A / n and every
    earlier one >= 1e-3 tr A / n, so rounding cannot move the column."""
    for k in cr.status_columns(n):
        A = cr.indefinite_at(n, k, 4000 + n)
        assert np.array_equal(A, A.T)
        _, status, piv = cr.chol_ld(A)
        assert status == k + 1
        assert piv[k] <= -1e-3 / n
        assert np.all(piv[:k] >= 1e-3 / n)


@pytest.mark.parametrize("n", cr.CERT_ORDERS)
def test_certificate_inputs_are_decisive(n):
    """lambda_min = c TAU tr A: c = 0.5 fails and c = 2 passes in the reference, each with |last pivot| / tr A >= 1e-10
    where it decides (the refused matrix's first non-positive pivot; the admitted matrix's smallest pivot)."""
    A = cr.cert_case(n, 0.5)
    _, status, piv = cr.chol_ld(A, -cr.TAU)
    assert status != 0
    assert piv[status - 1] <= -1e-10
    assert np.all(piv[: status - 1] >= 1e-10)
    A = cr.cert_case(n, 2.0)
    _, status, piv = cr.chol_ld(A, -cr.TAU)
    assert status == 0
    assert piv.min() >= 1e-10


def test_bars_of_the_gpu_tests():
    """Every bar is a power of two, and the bar a test applies at a well-conditioned order n never exceeds 16 n u."""
    import math

    import test_chol_batch_gpu as tg

    for table in (tg.BARS_WELL, tg.BARS_GRADED):
        for bars in table.values():
            assert len(bars) == 3 and all(math.log2(b) == round(math.log2(b)) for b in bars)
    assert sorted(tg.BARS_WELL) == sorted(cr.WELL_GROUPS) and sorted(tg.BARS_GRADED) == sorted(cr.GRADED_GROUPS)
    assert sorted(tg.BARS_TRSM) == sorted(cr.TRSM_GROUPS)
    for group, orders in cr.WELL_GROUPS.items():
        for n in orders:
            assert all(b <= 16 * n * cr.U for b in tg.well_bars(n, group == "k32"))
