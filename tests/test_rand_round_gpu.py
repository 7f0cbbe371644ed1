"""GPU: the randomized rounding of TT sums -- the driver xrs_tt_round_randomized through capi and xe.sum_rounded /
xe.round_randomized (include/xerus/algorithms/randomizedRounding.h) -- against the NumPy restatement rand_round_ref.py
on the same random TT and against the existing operator+ / round path. The bounds that cite "the restatement's
recorded maximum" take it from test_rand_round_ref_cpu.py (200 seeds)."""
import numpy as np
import pytest

import rand_round_ref as rr
import random_ttsvd_ref as rt
from xerus_amd import capi

pytestmark = pytest.mark.gpu

# test_rand_round_ref_cpu.py: maxima over 200 seeds on the same fixtures
EXACT_RECOVERY_MAX = {0: 1.843e-13, 2: 6.70e-14, 8: 6.98e-14}
QUASI_OPTIMALITY_MAX = 1.6455
PARITY = 1e-6            # the project's parity bar
ROUNDING = 1e4 * 2.0 ** -53   # results that are exact up to rounding on small, well-conditioned inputs: 1.1e-12


def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _tt(xe, cores):
    t = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        t.set_component(k, _tensor(xe, c))
    return t


def _operator(xe, cores):
    A = xe.TTOperator([c.shape[1] for c in cores] + [c.shape[2] for c in cores])
    for k, c in enumerate(cores):
        A.set_component(k, _tensor(xe, c))
    return A


def _dense(xe, t):
    return xe.Tensor(t).to_ndarray()


def _cores(t):
    return [t.get_component(k).to_ndarray() for k in range(t.degree())]


@pytest.fixture(scope="module")
def exact():
    terms, coef, ranks = rr.exact_fixture()
    return terms, coef, ranks, rr.full_sum(terms, coef)


@pytest.fixture(scope="module")
def noisy():
    terms, coef, ranks = rr.noisy_fixture()
    return terms, coef, ranks, rr.full_sum(terms, coef)


@pytest.fixture(scope="module")
def ragged():
    terms, coef, ell = rr.ragged_fixture()
    return terms, coef, ell, rr.full_sum(terms, coef)


# ------------------------------------------------------------------------------------------ driver: parity, structure
def _driver(handle, terms, coef, ell, seed):
    dev = [capi.TTDevice.from_cores(handle, t) for t in terms]
    return handle.tt_round_randomized(dev, coef, ell, seed)


@pytest.mark.parametrize("which,seed", [("noisy", 11), ("ragged", 12), ("ragged", 2 ** 63 + 5)])
def test_parity_with_the_restatement(handle, noisy, ragged, which, seed):
    """The same Omega (G(seed, stream = k)) on both sides, Z of full rank: the projector Q Q^T is unique, so the dense
    sketch results agree whatever sign convention the QR has. Relative difference <= 1e-6."""
    terms, coef, ell, _ = noisy if which == "noisy" else ragged
    if which == "noisy":
        ell = [r + 8 for r in ell]   # the fixture carries the target ranks
    got = _driver(handle, terms, coef, ell, seed)
    want = rr.sketch_sum(terms, coef, ell, seed)
    diff = rr.rel_err(rt.tt_full(got.cores()), rt.tt_full(want))
    print(f"parity on the {which} fixture, seed {seed}: relative difference {diff:.3e}")
    assert diff <= PARITY


@pytest.mark.parametrize("which", ["noisy", "ragged"])
def test_structure(handle, noisy, ragged, which):
    """r_out is the capped l; cores 0 .. d-2 are orthonormal as (l_k n_k) x l_{k+1} matrices (the move_core tests'
    tolerance: ||Q^T Q - I||_F <= 1e-12 x columns)."""
    terms, coef, ell, _ = noisy if which == "noisy" else ragged
    if which == "noisy":
        ell = [r + 8 for r in ell]
    dims = [c.shape[1] for c in terms[0]]
    got = _driver(handle, terms, coef, ell, 21)
    assert got.r == rr.capped_ranks(dims, terms, ell)
    cores = got.cores()
    for c in cores[:-1]:
        Q = c.reshape(-1, c.shape[2])
        assert np.linalg.norm(Q.T @ Q - np.eye(Q.shape[1])) <= 1e-12 * Q.shape[1]


def test_driver_caps_and_degenerate_orders(handle):
    rng = np.random.default_rng(31)
    # d = 1: sum_j c_j Y_0 through the summed GEMM
    a, b = rt.random_tt((7,), (), rng), rt.random_tt((7,), (), rng)
    got = _driver(handle, [a, b], [2.0, -1.0], [], 1)
    assert got.r == [1, 1]
    assert np.abs(got.cores()[0] - (2.0 * a[0] - b[0])).max() <= 8 * 2.0 ** -53 * (2 * np.abs(a[0]) + np.abs(b[0])).max()
    # d = 2, l far above what the modes allow: capped at 3
    x, y = rt.random_tt((4, 3), (2,), rng), rt.random_tt((4, 3), (3,), rng)
    got = _driver(handle, [x, y], [1.0, 0.5], [50], 2)
    assert got.r == [1, 3, 1]
    assert rr.rel_err(rt.tt_full(got.cores()), rr.full_sum([x, y], [1.0, 0.5])) <= ROUNDING


def test_driver_argument_errors(handle):
    rng = np.random.default_rng(32)
    x = capi.TTDevice.from_cores(handle, rt.random_tt((4, 3, 5), (2, 2), rng))
    y = capi.TTDevice.from_cores(handle, rt.random_tt((4, 3, 4), (2, 2), rng))
    for terms, coef, ell in [([x], [1.0], [2]), ([x], [1.0, 2.0], [2, 2]), ([x, y], [1.0, 1.0], [2, 2]), ([], [], [2, 2]),
                             ([x], [1.0], [2, 0])]:
        with pytest.raises(capi.XrsError) as e:
            handle.tt_round_randomized(terms, coef, ell, 3)
        assert e.value.code == -1


# ------------------------------------------------------------------------------------------ xe.sum_rounded
@pytest.mark.parametrize("p", [0, 2, 8])
def test_exact_recovery(xe, exact, p):
    """z + 2.5 u - 2.5 u. Oversampling 2 and 8 put l above the exact rank: Z is rank deficient and xrs_qr takes its
    Householder route; bound 100 x the restatement's recorded maximum (and never looser than 1e-6). Oversampling 0
    (a square sketch can be ill conditioned): 1e-6. Exact ranks, canonicalized, core at 0."""
    terms, coef, ranks, full = exact
    xe.seed(300 + p)
    T = xe.sum_rounded([_tt(xe, t) for t in terms], coef, ranks, [p] * 4)
    assert T.ranks() == ranks
    assert T.canonicalized and T.corePosition == 0
    err = rr.rel_err(_dense(xe, T), full)
    bound = PARITY if p == 0 else min(100 * EXACT_RECOVERY_MAX[p], PARITY)
    print(f"exact recovery, oversampling {p}: relative error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_quasi_optimality(xe, noisy):
    """Oversampling 8 against (the same sum).round(ranks) of the existing path, which is the TT-SVD optimum to
    rounding: the error ratio stays within the restatement's recorded maximum x 1.05."""
    terms, coef, ranks, full = noisy
    tts = [_tt(xe, t) for t in terms]
    S = coef[0] * tts[0] + coef[1] * tts[1] + coef[2] * tts[2]
    S.round(ranks)
    best = rr.rel_err(_dense(xe, S), full)
    xe.seed(400)
    T = xe.sum_rounded(tts, coef, ranks, [8] * 4)
    assert T.ranks() == ranks
    err = rr.rel_err(_dense(xe, T), full)
    print(f"quasi-optimality: randomized {err:.4e}, operator+ and round {best:.4e}, ratio {err / best:.4f}")
    assert err <= 1.05 * QUASI_OPTIMALITY_MAX * best


def test_round_randomized_keeps_an_exact_input(xe, exact):
    terms, _, ranks, _ = exact
    x = _tt(xe, terms[0])
    xe.seed(500)
    T = xe.round_randomized(x, ranks, [2] * 4)
    assert T.ranks() == ranks and T.canonicalized and T.corePosition == 0
    err = rr.rel_err(_dense(xe, T), rt.tt_full(terms[0]))
    print(f"round_randomized of an exact input: relative error {err:.3e}")
    assert err <= min(100 * EXACT_RECOVERY_MAX[2], PARITY)


def test_operator_overload_agrees_with_the_tt_view(xe):
    rng = np.random.default_rng(41)
    n, m, ranks = (3, 2, 4), (2, 3, 2), [3, 2]

    def op_cores(r):
        rk = [1] + list(r) + [1]
        return [rng.standard_normal((rk[k], n[k], m[k], rk[k + 1])) for k in range(3)]

    a, b = op_cores((3, 2)), op_cores((2, 3))
    merged = lambda cs: [c.reshape(c.shape[0], -1, c.shape[3]) for c in cs]  # noqa: E731
    xe.seed(600)
    O = xe.sum_rounded([_operator(xe, a), _operator(xe, b)], [1.0, -2.0], ranks, [1, 1])
    xe.seed(600)
    T = xe.sum_rounded([_tt(xe, merged(a)), _tt(xe, merged(b))], [1.0, -2.0], ranks, [1, 1])
    assert O.ranks() == T.ranks() == ranks
    view = _dense(xe, T).reshape(3, 2, 2, 3, 4, 2).transpose(0, 2, 4, 1, 3, 5)
    assert rr.rel_err(_dense(xe, O), view) <= ROUNDING
    xe.seed(601)
    O1 = xe.round_randomized(_operator(xe, a), ranks, [1, 1])
    xe.seed(601)
    T1 = xe.round_randomized(_tt(xe, merged(a)), ranks, [1, 1])
    view1 = _dense(xe, T1).reshape(3, 2, 2, 3, 4, 2).transpose(0, 2, 4, 1, 3, 5)
    assert rr.rel_err(_dense(xe, O1), view1) <= ROUNDING


def test_degenerate_orders(xe):
    rng = np.random.default_rng(51)
    # d = 1
    a, b = rt.random_tt((7,), (), rng), rt.random_tt((7,), (), rng)
    T = xe.sum_rounded([_tt(xe, a), _tt(xe, b)], [2.0, -1.0], [], [])
    assert rr.rel_err(_dense(xe, T), rr.full_sum([a, b], [2.0, -1.0])) <= ROUNDING
    # d = 2, and ranks larger than the modes allow (l capped at 3)
    x, y = rt.random_tt((4, 3), (2,), rng), rt.random_tt((4, 3), (3,), rng)
    T = xe.sum_rounded([_tt(xe, x), _tt(xe, y)], [1.0, 0.5], [50], [4])
    assert T.ranks() == [3]
    assert rr.rel_err(_dense(xe, T), rr.full_sum([x, y], [1.0, 0.5])) <= ROUNDING
    # a single term with a coefficient
    z = rt.random_tt((4, 3, 5), (3, 4), rng)
    T = xe.sum_rounded([_tt(xe, z)], [-3.0], [3, 4], [0, 0])
    assert T.ranks() == [3, 4]
    assert rr.rel_err(_dense(xe, T), -3.0 * rt.tt_full(z)) <= PARITY   # square sketches: the parity bar


def test_seeding(xe, noisy):
    terms, coef, ranks, _ = noisy
    tts = [_tt(xe, t) for t in terms]
    xe.seed(7)
    a = _cores(xe.sum_rounded(tts, coef, ranks, [4] * 4))
    b = _cores(xe.sum_rounded(tts, coef, ranks, [4] * 4))
    xe.seed(7)
    c = _cores(xe.sum_rounded(tts, coef, ranks, [4] * 4))
    assert all(np.array_equal(u, v) for u, v in zip(a, c))
    assert not all(np.array_equal(u, v) for u, v in zip(a, b))


def test_argument_errors(xe, exact):
    terms, coef, ranks, _ = exact
    tts = [_tt(xe, t) for t in terms]
    other = _tt(xe, rt.random_tt((6, 5, 4, 5, 5), (2, 2, 2, 2), np.random.default_rng(1)))
    with pytest.raises(RuntimeError):
        xe.sum_rounded([], [], ranks, [2] * 4)
    with pytest.raises(RuntimeError):
        xe.sum_rounded(tts, coef[:2], ranks, [2] * 4)
    with pytest.raises(RuntimeError):
        xe.sum_rounded(tts, coef, ranks[:3], [2] * 4)
    with pytest.raises(RuntimeError):
        xe.sum_rounded(tts, coef, ranks, [2] * 5)
    with pytest.raises(RuntimeError):
        xe.sum_rounded(tts[:2] + [other], coef, ranks, [2] * 4)
    with pytest.raises(RuntimeError):
        xe.round_randomized(tts[0], ranks[:2], [2] * 4)
