"""The NumPy restatement of the randomized rounding of TT sums (rand_round_ref.py) on the CPU, with the device's
Gaussian matrix G(seed, stream) (fp32-rounded Philox normals). The maxima recorded here are the yardsticks the GPU
tests (test_rand_round_gpu.py) cite."""
import numpy as np
import pytest

import rand_round_ref as rr
import random_ttsvd_ref as rt

SEEDS = range(200)

# Maxima over SEEDS as the tests below print them (pytest -s), recorded for the GPU tests' bounds
EXACT_RECOVERY_MAX = 1.843e-13    # oversampling 0; 6.70e-14 at oversampling 2, 6.98e-14 at 8
QUASI_OPTIMALITY_MAX = 1.6455     # oversampling 8 (median 1.116)
# What "recovered" is held to here: the terms are up to 2.5 ||u|| + ||z|| ~ 1.9 ||z|| large and cancel, each of the
# five cores passes through two products with random cores of condition ~1e2, so errors of some 1e4 u relative to
# ||z|| are rounding and nothing else; 1e5 u = 1.1e-11 separates that from any truncation (the smallest singular
# value kept is ~1e-2 relative).
EXACT_RECOVERY_BOUND = 1e5 * 2.0 ** -53


@pytest.fixture(scope="module")
def exact():
    terms, coef, ranks = rr.exact_fixture()
    return terms, coef, ranks, rr.full_sum(terms, coef)


@pytest.fixture(scope="module")
def noisy():
    terms, coef, ranks = rr.noisy_fixture()
    full = rr.full_sum(terms, coef)
    best = rr.rel_err(rt.tt_full(rt.tt_svd(full, ranks)), full)
    return terms, coef, ranks, full, best


@pytest.mark.parametrize("p", [0, 2, 8])
def test_exact_recovery(exact, p):
    """z + 2.5 u - 2.5 u (z of ranks 6,7,7,6, u of rank 5, dims (6,5,4,5,6)) is recovered with oversampling 0, 2, 8.
    Maximum relative error over 200 seeds: 1.843e-13 (p = 0), 6.70e-14 (p = 2), 6.98e-14 (p = 8), recorded as
    EXACT_RECOVERY_MAX; asserted below EXACT_RECOVERY_BOUND = 1e5 u (reasoned above)."""
    terms, coef, ranks, full = exact
    worst = 0.0
    for seed in SEEDS:
        cores = rr.sum_rounded(terms, coef, ranks, [p] * 4, seed)
        assert [c.shape[2] for c in cores[:-1]] == ranks
        worst = max(worst, rr.rel_err(rt.tt_full(cores), full))
    print(f"exact recovery, oversampling {p}: max rel err over {len(SEEDS)} seeds = {worst:.3e}")
    assert worst <= EXACT_RECOVERY_BOUND


def test_quasi_optimality(noisy):
    """z + 1e-3 ||z|| (a / ||a|| + b / ||b||), a and b of ranks 6,9,9,6, rounded to (6,7,7,6) with oversampling 8: the
    error is within a factor 2 of the TT-SVD's. Maximum ratio over 200 seeds: 1.6455, median 1.116 (recorded as
    QUASI_OPTIMALITY_MAX); the TT-SVD's relative error is 1.281e-03."""
    terms, coef, ranks, full, best = noisy
    ratios = []
    for seed in SEEDS:
        cores = rr.sum_rounded(terms, coef, ranks, [8] * 4, seed)
        ratios.append(rr.rel_err(rt.tt_full(cores), full) / best)
    print(f"quasi-optimality, oversampling 8: TT-SVD error {best:.3e}, ratio max {max(ratios):.4f} median {np.median(ratios):.4f}")
    assert max(ratios) <= 2.0


@pytest.mark.parametrize("seed", [0, 7])
def test_independent_of_the_split_into_terms(noisy, seed):
    """One term holding the block-diagonal sum gives the same tensor as the three terms, to rounding: W and X of the
    block term are the stacked W^(j) and the concatenated X^(j), so Z and every later quantity agree."""
    terms, coef, ranks, full, _ = noisy
    ell = [r + 8 for r in ranks]
    three = rt.tt_full(rr.sketch_sum(terms, coef, ell, seed))
    one = rt.tt_full(rr.sketch_sum([rr.block_sum(terms, coef)], [1.0], ell, seed))
    assert rr.rel_err(one, three) <= 1e-12
    assert rr.rel_err(three, full) <= 1e-2


def test_sketch_structure(noisy):
    terms, coef, ranks, _, _ = noisy
    cores = rr.sketch_sum(terms, coef, [r + 8 for r in ranks], 3)
    assert [c.shape[0] for c in cores] + [1] == rr.capped_ranks(rr.DIMS, terms, [r + 8 for r in ranks]) == [1, 6, 15, 15, 6, 1]
    for c in cores[:-1]:
        q = c.reshape(-1, c.shape[2])
        assert np.abs(q.T @ q - np.eye(q.shape[1])).max() <= 1e-13


def test_degenerate_orders():
    rng = np.random.default_rng(5)
    a, b = rt.random_tt((7,), (), rng), rt.random_tt((7,), (), rng)
    assert np.allclose(rr.sum_rounded([a, b], [2.0, -1.0], [], [])[0], 2.0 * a[0] - b[0], rtol=0, atol=1e-15)
    x, y = rt.random_tt((4, 3), (2,), rng), rt.random_tt((4, 3), (3,), rng)
    got = rt.tt_full(rr.sum_rounded([x, y], [1.0, 0.5], [50], [4]))   # capped by the mode sizes: 3
    assert rr.rel_err(got, rr.full_sum([x, y], [1.0, 0.5])) <= 1e-14
