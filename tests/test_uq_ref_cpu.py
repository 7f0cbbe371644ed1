"""CPU: pins tests/uq_ref.py, the NumPy restatement of the reference's UQ-ADF (uqAdf.cpp) that the GPU tests
(test_uq_adf_gpu.py) compare against."""
import numpy as np
import pytest

import uq_ref


def test_hermite_closed_forms():
    v = np.linspace(-6.0, 6.0, 49)
    p = uq_ref.hermite(v, 5)
    want = np.stack([np.ones_like(v), v, v ** 2 - 1, v ** 3 - 3 * v, v ** 4 - 6 * v ** 2 + 3], axis=1)
    assert np.abs(p - want).max() <= 1e-14 * np.abs(want).max()
    assert uq_ref.hermite(0.5, 1).tolist() == [1.0]
    assert uq_ref.hermite(0.5, 2).tolist() == [1.0, 0.5]


def test_evaluate_is_the_contraction_with_the_basis():
    true, rv, sols, _ = uq_ref.make_case([5, 3, 4], [2, 3], 9, 4)
    want = np.einsum('nst,js,jt->jn', true.full(), uq_ref.hermite(rv[:, 0], 3), uq_ref.hermite(rv[:, 1], 4))
    assert np.abs(sols - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("dims,ranks,N,seed", uq_ref.FULL_SOLVE_CASES)
def test_full_solve_converges(dims, ranks, N, seed):
    true, rv, sols, x = uq_ref.make_case(dims, ranks, N, seed)
    hist = uq_ref.uq_adf(x, rv, sols)
    assert len(hist) < 1000
    assert hist[-1] <= 1e-13
    err = np.linalg.norm(x.full() - true.full()) / np.linalg.norm(true.full())
    assert err <= 1e-13


def test_mc_stream_order_and_scaling(ref):
    x = ref.TT.random([6, 3, 4], [3, 2], ref.Rng(11))
    rv0, _ = uq_ref.uq_mc(x, 5, 0)
    rv1, s1 = uq_ref.uq_mc(x, 5, 1)
    stream = ref.Rng(5489).normal(10)
    # sample-major; within a sample the draw for mode 2 comes before the one for mode 1
    assert rv0[0, 1] == stream[0] and rv0[0, 0] == stream[1] and rv0[1, 1] == stream[2]
    assert np.array_equal(rv1[:, 0], 0.3 * rv0[:, 0]) and np.array_equal(rv1[:, 1], rv0[:, 1])
    assert np.allclose(uq_ref.uq_avg(x, 5, 1), s1.mean(axis=0), rtol=1e-14, atol=0)


def test_initialisation_reproduces_mean_and_linear_terms(ref):
    """uq_adf_initial: at xi = 0 the start is the mean (He_1(0) = 0). The m-th term carries He_0 in mode m and
    He_1 in every other stochastic mode (uqAdf.cpp:376-381, kept as the reference has it), so with two
    stochastic modes the m-th difference is scaled by the OTHER variable. The rounding at 0.00025 cuts nothing
    of this rank-3 sum; 1e-3 is four times its threshold."""
    dims = [6, 3, 3]
    _, rv, sols, _ = uq_ref.make_case(dims, [2, 2], 30, 9)
    init_rv = np.diag([1.0, 2.0])
    init_sols = np.random.default_rng(9).standard_normal((2, 6))
    x = uq_ref.uq_adf_initial(dims, rv, sols, init_rv, init_sols)
    mean = sols.mean(axis=0)
    at = uq_ref.evaluate(x, np.array([[0.0, 0.0], [0.5, 0.0], [0.0, -1.5]]))
    scale = np.abs(sols).max()
    assert np.abs(at[0] - mean).max() <= 1e-3 * scale
    assert np.abs(at[1] - (mean + 0.5 * (init_sols[1] - mean))).max() <= 1e-3 * scale
    assert np.abs(at[2] - (mean - 1.5 * (init_sols[0] - mean))).max() <= 1e-3 * scale
