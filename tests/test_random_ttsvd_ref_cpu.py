"""CPU: the NumPy restatement of tests/random_ttsvd_ref.py -- Philox4x32-10 against the Random123 known answers,
the statistics of the fp64 normal formula, and the restated randomTTSVD / decomposition_als on the inputs of the
GPU tests (the bounds asserted there rest on the values checked here)."""
import numpy as np
import pytest

import random_ttsvd_ref as rr

# Random123 (kat_vectors, philox4x32 with 10 rounds): counter, key, output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    got = rr.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]


def test_words_layout():
    """W(i, q): key = (seed low, seed high), counter = (q low, q high, i, stream)."""
    seed, stream = (0xA4093822 | (0x299F31D0 << 32)), 0x03707344
    w = rr.words(seed, stream, 3, 5)
    assert w.shape == (3, 5, 4) and w.dtype == np.uint32
    for i, q in ((0, 0), (2, 4), (1, 3)):
        one = rr.philox4x32_10(np.array([q, 0, i, stream], dtype=np.uint64),
                               np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
        assert np.array_equal(w[i, q], one)


def test_normal_formula_statistics():
    """5 sigma bounds on 64 x 4096 normals: mean, variance, and the correlation of any two of 8 rows."""
    g = rr.gaussian_matrix(seed=20261020, stream=3, s=64, m=4096)
    N = g.size
    assert abs(g.mean()) < 5 / np.sqrt(N)
    assert abs(g.var() - 1.0) < 5 * np.sqrt(2.0 / N)
    rows = g[:8]
    corr = rows @ rows.T / 4096
    off = corr - np.diag(np.diag(corr))
    assert np.max(np.abs(off)) < 5 / np.sqrt(4096)
    assert np.max(np.abs(g)) <= np.sqrt(64 * np.log(2.0))   # the tail stops at 6.66


def test_prefix_property():
    big = rr.gaussian_matrix(5, 1, 17, 130)
    assert np.array_equal(rr.gaussian_matrix(5, 1, 5, 37), big[:5, :37])
    assert not np.array_equal(rr.gaussian_matrix(5, 2, 5, 37), big[:5, :37])
    assert not np.array_equal(rr.gaussian_matrix(6, 1, 5, 37), big[:5, :37])


def _rel(cores, x):
    return np.linalg.norm(rr.tt_full(cores) - x) / np.linalg.norm(x)


SEEDS = range(1, 9)


def test_exact_rank_input():
    """Ranks (3,4,4,2) come back exactly; 1e-12 with oversampling 2, 1e-6 with none (a square sketch can be ill
    conditioned). The GPU test asserts the same two bounds."""
    x = rr.exact_rank_tensor()
    worst2 = worst0 = 0.0
    for seed in SEEDS:
        c2 = rr.random_ttsvd(x, rr.EXACT_RANKS, [2] * 4, seed)
        assert tuple(c.shape[2] for c in c2[:-1]) == rr.EXACT_RANKS
        worst2 = max(worst2, _rel(c2, x))
        c0 = rr.random_ttsvd(x, rr.EXACT_RANKS, [0] * 4, seed)
        assert tuple(c.shape[2] for c in c0[:-1]) == rr.EXACT_RANKS
        worst0 = max(worst0, _rel(c0, x))
    print("exact rank: worst relative error %.3g (oversampling 2), %.3g (oversampling 0)" % (worst2, worst0))
    assert worst2 <= 1e-12
    assert worst0 <= 1e-6


@pytest.mark.parametrize("rank", [3, 2])
def test_quasi_optimality(rank):
    """Hilbert-type tensor, oversampling 4: within 1.01 of the TT-SVD's error."""
    y = rr.hilbert_tensor()
    ranks = [rank] * 4
    best = np.linalg.norm(rr.tt_full(rr.tt_svd(y, ranks)) - y)
    worst = 0.0
    for seed in SEEDS:
        err = np.linalg.norm(rr.tt_full(rr.random_ttsvd(y, ranks, [4] * 4, seed)) - y)
        worst = max(worst, err / best)
    print("rank %d: worst error ratio to TT-SVD %.9f" % (rank, worst))
    assert worst <= 1.01


def test_shapes():
    rng = np.random.default_rng(7)
    v = rng.standard_normal(5)
    assert np.array_equal(rr.tt_full(rr.random_ttsvd(v, [], [])), v)
    m = rng.standard_normal((4, 6))
    assert _rel(rr.random_ttsvd(m, [4], [3], 1), m) < 1e-12          # s capped at M = 4
    t = rr.tt_full(rr.random_tt((3, 1, 4, 2), (2, 2, 2), rng))
    assert _rel(rr.random_ttsvd(t, [2, 2, 2], [2, 2, 2], 1), t) < 1e-12   # a mode of size 1
    f = rng.standard_normal((3, 1, 4, 2))                                # full rank: the maximal ranks (3, 3, 2)
    c = rr.random_ttsvd(f, [50, 50, 50], [1, 1, 1], 1)                   # asked for more than that
    assert [k.shape[2] for k in c[:-1]] == [3, 3, 2] and _rel(c, f) < 1e-12


ALS_DIMS = (2,) * 14


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_decomposition_als_reference_unit_test(seed):
    """src/unitTests/decompositionAls.cxx:27-43: d = 14, n = 2, rank 4 target and start; ||X - B|| < 1e-8."""
    rng = np.random.default_rng(seed)
    target = rr.random_tt(ALS_DIMS, [4] * 13, rng)
    rr.move_core(target, 0)
    b = rr.tt_full(target)
    start = rr.random_tt(ALS_DIMS, [4] * 13, rng)
    rr.move_core(start, 0)
    cores, residuals = rr.decomposition_als(start, b)
    print("seed %d: %d sweeps, residual %.3g -> %.3g" % (seed, len(residuals) - 1, residuals[0], residuals[-1]))
    assert residuals[-1] < 1e-8
    assert np.linalg.norm(rr.tt_full(cores) - b) < 1e-8


def test_decomposition_als_is_monotone_after_a_sketch():
    y = rr.hilbert_tensor()
    start = rr.random_ttsvd(y, [3] * 4, [0] * 4, 5)
    _, residuals = rr.decomposition_als(start, y)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(residuals, residuals[1:]))
    assert residuals[-1] <= residuals[0]
