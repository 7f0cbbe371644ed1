"""CPU: pins tests/riemannian_ref.py, the NumPy restatement the GPU tests of the Riemannian algorithms compare
against, on a shape small enough for dense linear algebra: modes [2, 3, 2], ranks [2, 2].

The tangent space at X is spanned by the TTs with one component of X replaced by a unit tensor -- the
construction of the reference's own test (unitTests/retractions.cxx:163-178) -- so the restatement's projection
must equal the dense orthogonal projector onto that span. Tolerance 1e-12 (the Grams' condition numbers here are
below 1e2, so cond * 2^-52 leaves four digits of room)."""
import numpy as np
import pytest

import riemannian_ref as rr
from oracle import xerus_ref as ref

DIMS, RANKS = [2, 3, 2], [2, 2]


def _random_tt(rng, dims, ranks, canonical=True):
    r = [1] + list(ranks) + [1]
    tt = ref.TT([rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))])
    if canonical:
        tt.move_core(0)
    return tt


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(7)
    X = _random_tt(rng, DIMS, RANKS)
    Z = _random_tt(rng, DIMS, RANKS, canonical=False)
    basis = []
    for n, c in enumerate(X.cores):
        for i in range(c.size):
            cores = [k.copy() for k in X.cores]
            e = np.zeros(c.size)
            e[i] = 1.0
            cores[n] = e.reshape(c.shape)
            basis.append(ref.TT(cores).full().reshape(-1))
    B = np.array(basis).T
    P = B @ np.linalg.pinv(B)
    return X, Z, P, rr.project(X.cores, Z.cores)


def test_projection_is_the_dense_orthogonal_projector(case):
    X, Z, P, t = case
    want = (P @ Z.full().reshape(-1)).reshape(DIMS)
    assert _rel(rr.full(t), want) <= 1e-12


def test_gauge_condition_and_idempotence(case):
    X, Z, P, t = case
    scale = rr.frob_norm(t)   # (the last component is zero in exact arithmetic: its core is square)
    for k in range(1, len(DIMS)):
        assert np.linalg.norm(np.einsum('arj,brj->ab', t.components[k], X.cores[k])) <= 1e-14 * scale
    again = rr.project(X.cores, rr.to_tt(t).cores)
    assert _rel(rr.full(again), rr.full(t)) <= 1e-12


def test_block_tt_and_added_to_base(case):
    X, Z, P, t = case
    assert _rel(ref.TT(rr.block_cores(t.base, t.components, False)).full(), rr.full(t)) <= 1e-12
    assert _rel(rr.to_tt(t).full(), rr.full(t)) <= 1e-12
    assert _rel(rr.to_tt(t, add_base=True).full(), X.full() + rr.full(t)) <= 1e-12
    assert [c.shape for c in rr.block_cores(t.base, t.components, True)] == [(1, 2, 4), (4, 3, 4), (4, 2, 1)]


def test_scalar_product_is_the_embedded_one(case):
    X, Z, P, t = case
    rng = np.random.default_rng(8)
    t2 = rr.project(X.cores, _random_tt(rng, DIMS, [1, 2], canonical=False).cores)
    assert rr.scalar_product(t, t2) == pytest.approx(float(np.vdot(rr.full(t), rr.full(t2))), rel=1e-12)
    assert rr.frob_norm(t) == pytest.approx(float(np.linalg.norm(rr.full(t))), rel=1e-12)


def test_retractions_are_first_order(case):
    """Every retraction moves X by the (small) tangent change up to second order and keeps the ranks."""
    X, Z, P, t = case
    eps = 1e-4
    small = t.scaled(eps / rr.frob_norm(t))
    change = rr.to_tt(small)
    want = X.full() + rr.full(small)
    for retraction, arg in [(rr.hosvd_retraction(2), small), (rr.hosvd_retraction(2), change), (rr.hosvd_retraction_keep, small),
                            (rr.als_retraction, small), (rr.als_retraction, change), (rr.submanifold_retraction, small),
                            (rr.submanifold_retraction, change)]:
        Y = X.copy()
        retraction(Y, arg)
        assert list(Y.ranks) == RANKS
        assert np.linalg.norm(Y.full() - want) <= 10 * eps * eps


def test_transport_to_the_same_base_is_the_identity(case):
    X, Z, P, t = case
    moved = rr.projective_transport(X, t)
    for a, b in zip(moved.components, t.components):
        assert np.linalg.norm(a - b) <= 1e-12 * max(1.0, np.linalg.norm(b))


def test_solver_loops_reduce_the_residual():
    """Steepest descent on min ||x - b||, b of the ranks of x, converges to b; the geometric CG never increases
    the residual (its line search only accepts decreases; the reference's step length grows by at most 1 / 0.8
    per step, steepestDescent.cpp:43-63, so its start is slow by construction)."""
    rng = np.random.default_rng(3)
    dims, ranks = [3, 3, 3], [2, 2]
    b = _random_tt(rng, dims, ranks)
    x0 = _random_tt(rng, dims, ranks)
    nb = rr.tt_norm(b)
    x = x0.copy()
    hist = rr.steepest_descent(None, x, b, 30, 1e-10, rr.submanifold_retraction)
    assert all(b2 <= a2 * (1 + 1e-12) for a2, b2 in zip(hist, hist[1:]))
    assert hist[-1] <= 1e-6 * nb
    assert np.linalg.norm(x.full() - b.full()) == pytest.approx(hist[-1], abs=1e-9 * nb)
    x = x0.copy()
    hist = rr.geometric_cg(None, x, b, 30, 1e-12)
    assert all(b2 <= a2 for a2, b2 in zip(hist, hist[1:]))
    assert hist[-1] <= 0.5 * hist[0]
    assert np.linalg.norm(x.full() - b.full()) == pytest.approx(hist[-1], rel=1e-9)
