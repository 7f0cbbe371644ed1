"""GPU: xe.randomTTSVD and xe.decomposition_als (include/xerus/algorithms/randomSVD.h, decompositionAls.h;
reference randomSVD.h:31-98, decompositionAls.cpp:36-65, unit test src/unitTests/decompositionAls.cxx:27-43).
The bounds are those of the NumPy restatement, checked on the CPU in test_random_ttsvd_ref_cpu.py."""
import numpy as np
import pytest

import random_ttsvd_ref as rr

pytestmark = pytest.mark.gpu


def _dense(xe, t):
    return xe.Tensor(t).to_ndarray()


def _cores(t):
    return [t.get_component(k).to_ndarray() for k in range(t.degree())]


@pytest.fixture(scope="module")
def exact(xe):
    x = rr.exact_rank_tensor()
    return x, xe.Tensor.from_ndarray(x)


@pytest.fixture(scope="module")
def hilbert(xe):
    y = rr.hilbert_tensor()
    return y, xe.Tensor.from_ndarray(y)


# ------------------------------------------------------------------------------------------ exact rank
def test_exact_rank_is_recovered(xe, exact):
    """Ranks (3,4,4,2), oversampling 2: exactly those ranks, core at 0, relative error <= 1e-12 (the restatement
    with fp32-rounded normals: 6.0e-15 at most over 200 seeds). Every sketch has two rows more than b has rank, so
    xrs_rq's route for rank-deficient input is exercised too."""
    x, X = exact
    xe.seed(101)
    T = xe.randomTTSVD(X, list(rr.EXACT_RANKS), [2, 2, 2, 2])
    assert tuple(T.ranks()) == rr.EXACT_RANKS
    assert T.canonicalized and T.corePosition == 0
    assert T.dimensions == list(rr.EXACT_DIMS)
    err = np.linalg.norm(_dense(xe, T) - x) / np.linalg.norm(x)
    print("exact rank, oversampling 2: relative error %.3e" % err)
    assert err <= 1e-12


def test_exact_rank_without_oversampling(xe, exact):
    """Oversampling 0: a square sketch can be ill conditioned (restatement: 6.9e-13 at most); the project's bar of
    1e-6."""
    x, X = exact
    xe.seed(102)
    T = xe.randomTTSVD(X, list(rr.EXACT_RANKS), [0, 0, 0, 0])
    assert tuple(T.ranks()) == rr.EXACT_RANKS
    err = np.linalg.norm(_dense(xe, T) - x) / np.linalg.norm(x)
    print("exact rank, oversampling 0: relative error %.3e" % err)
    assert err <= 1e-6


# ------------------------------------------------------------------------------------------ quasi-optimality
@pytest.mark.parametrize("rank", [3, 2])
def test_quasi_optimal_on_hilbert_tensor(xe, hilbert, rank):
    """Oversampling 4: the error is within 1.01 of the TT-SVD constructor's (restatement: 1 + 1.7e-7 at rank 3,
    1 + 1.4e-6 at rank 2)."""
    y, Y = hilbert
    ranks = [rank] * 4
    best = np.linalg.norm(_dense(xe, xe.TTTensor(Y, 0.0, ranks)) - y)
    xe.seed(200 + rank)
    T = xe.randomTTSVD(Y, ranks, [4] * 4)
    assert T.ranks() == ranks
    err = np.linalg.norm(_dense(xe, T) - y)
    print("rank %d: error %.6e, TT-SVD %.6e, ratio %.9f" % (rank, err, best, err / best))
    assert err <= 1.01 * best


# ------------------------------------------------------------------------------------------ seeding
def test_seeding(xe, hilbert):
    _, Y = hilbert
    xe.seed(7)
    a = _cores(xe.randomTTSVD(Y, [3] * 4, [2] * 4))
    c = _cores(xe.randomTTSVD(Y, [3] * 4, [2] * 4))   # no reseeding: another sketch
    xe.seed(7)
    b = _cores(xe.randomTTSVD(Y, [3] * 4, [2] * 4))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert any(not np.array_equal(p, q) for p, q in zip(a, c))


# ------------------------------------------------------------------------------------------ shapes
def _rel(xe, T, x):
    return np.linalg.norm(_dense(xe, T) - x) / np.linalg.norm(x)


def test_degree_one_and_two(xe):
    rng = np.random.default_rng(3)
    v = rng.standard_normal(5)
    T = xe.randomTTSVD(xe.Tensor.from_ndarray(v), [], [])
    assert T.degree() == 1 and T.canonicalized and T.corePosition == 0
    assert np.array_equal(_dense(xe, T), v)
    m = rng.standard_normal((7, 6))
    T = xe.randomTTSVD(xe.Tensor.from_ndarray(m), [6], [0])
    assert T.ranks() == [6] and _rel(xe, T, m) < 1e-6


def test_mode_of_size_one(xe):
    t = rr.tt_full(rr.random_tt((3, 1, 4, 2), (2, 2, 2), np.random.default_rng(4)))
    T = xe.randomTTSVD(xe.Tensor.from_ndarray(t), [2, 2, 2], [2, 2, 2])
    assert T.ranks() == [2, 2, 2] and _rel(xe, T, t) < 1e-6


def test_ranks_above_the_maximal_ranks_are_capped(xe):
    f = np.random.default_rng(5).standard_normal((3, 1, 4, 2))
    T = xe.randomTTSVD(xe.Tensor.from_ndarray(f), [50, 50, 50], [1, 1, 1])
    assert T.ranks() == xe.TTTensor.reduce_to_maximal_ranks([50, 50, 50], [3, 1, 4, 2]) == [3, 3, 2]
    assert _rel(xe, T, f) < 1e-6


def test_sketch_rows_are_capped_at_the_rows_of_the_unfolding(xe):
    """s_j = rank + oversampling > M_j = n_1 .. n_{j-1} at every step."""
    f = np.random.default_rng(6).standard_normal((2, 3, 40))
    T = xe.randomTTSVD(xe.Tensor.from_ndarray(f), [2, 6], [30, 30])
    assert T.ranks() == [2, 6] and _rel(xe, T, f) < 1e-6


def test_bad_arguments(xe, hilbert):
    _, Y = hilbert
    with pytest.raises(RuntimeError):
        xe.randomTTSVD(Y, [3] * 3, [2] * 4)
    with pytest.raises(RuntimeError):
        xe.randomTTSVD(Y, [3] * 4, [2] * 5)
    with pytest.raises(RuntimeError):
        xe.randomTTSVD(Y, [3, 0, 3, 3], [2] * 4)


# ------------------------------------------------------------------------------------------ decomposition_als
def test_decomposition_als_reference_unit_test(xe):
    """decompositionAls.cxx:27-43: d = 14, n = 2, B the dense tensor of a random rank-4 TT, X a random rank-4 start;
    ||X - B|| < 1e-8 after decomposition_als(X, B). The restatement reaches the bar from every start tried
    (test_random_ttsvd_ref_cpu.py), so the seed is not special."""
    xe.seed(0xBAADF00D)
    dims = [2] * 14
    B = xe.Tensor(xe.TTTensor.random(dims, 4))
    X = xe.TTTensor.random(dims, 4)
    xe.decomposition_als(X, B)
    res = np.linalg.norm(_dense(xe, X) - B.to_ndarray())
    print("decomposition_als: ||X - B|| = %.3e (||B|| = %.3e)" % (res, xe.frob_norm(B)))
    assert X.ranks() == xe.TTTensor.reduce_to_maximal_ranks([4] * 13, dims)
    assert res < 1e-8


def test_decomposition_als_does_not_increase_the_residual(xe, hilbert):
    """Started from randomTTSVD with no oversampling: ALS steps are monotone."""
    y, Y = hilbert
    xe.seed(11)
    T = xe.randomTTSVD(Y, [3] * 4, [0] * 4)
    before = np.linalg.norm(_dense(xe, T) - y)
    xe.decomposition_als(T, Y)
    after = np.linalg.norm(_dense(xe, T) - y)
    print("residual %.6e -> %.6e" % (before, after))
    assert T.ranks() == [3] * 4
    assert after <= before
