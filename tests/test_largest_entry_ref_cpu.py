"""CPU: the restatement of find_largest_entry (tests/largest_entry_ref.py) and the closed-form symmetric-square
cores the GPU tests compare against."""
import numpy as np
import pytest

import largest_entry_ref as ler
from oracle import xerus_ref as ref


@pytest.fixture(scope="module")
def fixtures():
    """(TT, dense) per fixture, built once; the tests copy before they change anything."""
    out = []
    for dims, ranks, seed in ler.FIXTURES:
        x = ler.make_fixture(dims, ranks, seed)
        out.append((x, x.full()))
    return out


def test_pair_index_is_a_bijection():
    for r in (1, 2, 3, 4, 17):
        assert [ler.pair_index(a, b, r) for a, b in ler.pairs(r)] == list(range(ler.sym_rank(r)))


def test_symmetric_square_cores_reproduce_the_square():
    """The closed-form cores represent f o f (1e-14 relative Frobenius) with ranks r (r + 1) / 2."""
    x = ref.TT.random_raw([3, 4, 2, 3], [3, 4, 2], ref.Rng(5))
    z = ref.TT([ler.symmetric_square_core(c) for c in x.cores])
    assert z.ranks == [6, 10, 3]
    assert ler.kronecker_square(x).ranks == [9, 16, 4]
    f = x.full()
    assert np.linalg.norm(z.full() - f * f) / np.linalg.norm(f * f) <= 1e-14


def test_symmetric_square_boundary_and_rank_one():
    """Rank 1 on a side gives s = 1; a rank-one TT squares entry by entry."""
    x = ref.TT.random_raw([3, 2, 4], [2, 1], ref.Rng(7))
    z = ref.TT([ler.symmetric_square_core(c) for c in x.cores])
    assert [c.shape for c in z.cores] == [(1, 3, 3), (3, 2, 1), (1, 4, 1)]
    f = x.full()
    assert np.linalg.norm(z.full() - f * f) / np.linalg.norm(f * f) <= 1e-14
    assert np.array_equal(z.cores[2], x.cores[2] * x.cores[2])


def test_fixture_gaps(fixtures):
    """Every fixture's gap ratio is <= 0.9: the condition under which the GPU test demands the exact position."""
    for (dims, ranks, seed), (_, full) in zip(ler.FIXTURES, fixtures):
        _, _, alpha = ler.gap(full)
        assert alpha <= 0.9, (dims, ranks, seed, alpha)


@pytest.mark.parametrize("square", [ler.kronecker_square, ler.symmetric_square], ids=["kronecker", "symmetric"])
@pytest.mark.parametrize("case", range(len(ler.FIXTURES)), ids=ler.FIXTURE_IDS)
def test_restatement_finds_the_argmax(fixtures, case, square):
    x, full = fixtures[case]
    pos, largest, alpha = ler.gap(full)
    before = [c.copy() for c in x.cores]
    got = ler.find_largest_entry(x.copy(), alpha, abs(largest), square=square)
    assert got == pos
    assert all(np.array_equal(a, b) for a, b in zip(before, x.cores))


def test_symmetric_square_keeps_the_ranks_lower(fixtures):
    """On the first fixture the largest rank before the threshold is smaller with the symmetric square."""
    x, full = fixtures[0]
    _, largest, alpha = ler.gap(full)
    tk, ts = [], []
    ler.find_largest_entry(x.copy(), alpha, abs(largest), square=ler.kronecker_square, trace=tk)
    ler.find_largest_entry(x.copy(), alpha, abs(largest), square=ler.symmetric_square, trace=ts)
    assert max(ts) <= max(tk)


def test_rank_one_position_first_index_wins():
    x = ref.TT([np.array([1.0, -2.0, 2.0]).reshape(1, 3, 1), np.array([-3.0, 3.0]).reshape(1, 2, 1)])
    assert ler.rank_one_position(x) == 1 * 2 + 0
