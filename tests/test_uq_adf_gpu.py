"""UQ-ADF (algorithms/uqAdf.h: uq_adf, uq_mc, uq_avg, UQMeasurementSet) on the GPU against the NumPy restatement of
the reference (tests/uq_ref.py, uqAdf.cpp:40-477).

Both sides start from the same cores and run the same sweeps, so residual histories and represented tensors are
compared (the cores' orthogonal gauge after move_core differs, as for every factorisation).
"""
import numpy as np
import pytest

import uq_ref

pytestmark = pytest.mark.gpu


def _tt_from(xe, cores):
    x = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        x.set_component(k, xe.Tensor.from_ndarray(np.ascontiguousarray(c)))
    return x


def _full(xe, x):
    return xe.Tensor(x).to_ndarray()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _tensors(xe, rows):
    return [xe.Tensor.from_ndarray(np.ascontiguousarray(r)) for r in rows]


@pytest.mark.parametrize("v", [-6.0, -0.3, 0.0, 2.5])
def test_randvar_to_position(xe, v):
    got = xe.randVar_to_position(v, 6).to_ndarray()
    want = uq_ref.hermite(v, 6)
    assert got.shape == (6,)
    assert np.all(np.abs(got - want) <= 1e-14 * np.maximum.accumulate(np.abs(want)))
    assert xe.randVar_to_position(v, 1).to_ndarray().tolist() == [1.0]


@pytest.mark.parametrize("dims,ranks,N,seed", [
    ([20, 5, 5, 4], [17, 16, 4], 257, 2),   # tiled congruence with ragged tiles at the interior positions
    ([6, 3, 4, 3], [4, 4, 2], 257, 7),
    ([5, 3], [2], 40, 3),                   # d = 2: no matrix stack
    ([5, 3, 4], [2, 3], 64, 4),             # d = 3: the first use of leftIs
    ([7, 4, 1, 3], [3, 1, 1], 50, 5),       # rank-1 edges and n_k = 1
])
def test_trajectory_matches_restatement(xe, dims, ranks, N, seed):
    """Six iterations from the same start: the residual history and the iterate of the restatement, at the
    1e-9 of test_adf_gpu.py for the same kind of comparison (on the CPU a 1e-14 perturbation of the start
    moves both by at most 4e-14 at these shapes)."""
    _, rv, sols, x0 = uq_ref.make_case(dims, ranks, N, seed)
    ox = x0.copy()
    ohist = uq_ref.uq_adf(ox, rv, sols, 6)
    x = _tt_from(xe, x0.cores)
    hist = xe.uq_adf(x, rv.tolist(), _tensors(xe, sols), 6)
    assert x.ranks() == ox.ranks
    assert len(hist) == len(ohist) == 6
    print("history rel dev %.3e, tensor rel dev %.3e" % (np.abs(np.asarray(hist) / np.asarray(ohist) - 1).max(),
                                                          _rel(_full(xe, x), ox.full())))
    assert np.all(np.abs(np.asarray(hist) - np.asarray(ohist)) <= 1e-9 * np.asarray(ohist))
    assert _rel(_full(xe, x), ox.full()) <= 1e-9


@pytest.mark.parametrize("dims,ranks,N,seed", uq_ref.FULL_SOLVE_CASES)
def test_full_solve_recovers_target(xe, ref, dims, ranks, N, seed):
    """The reference signature (1000 iterations, the reference's stopping rule). The stopping iteration depends
    on rounding at the noise floor, so the error against the target and the final residual are held to 1000 x
    the restatement's own values: the margin of another summation order at the floor."""
    true, rv, sols, x0 = uq_ref.make_case(dims, ranks, N, seed)
    ox = x0.copy()
    ohist = uq_ref.uq_adf(ox, rv, sols)
    full_true = true.full()
    oerr = _rel(ox.full(), full_true)
    x = _tt_from(xe, x0.cores)
    xe.uq_adf(x, rv.tolist(), _tensors(xe, sols))
    err = _rel(_full(xe, x), full_true)
    # the final residual of x, evaluated by the restatement
    res = np.linalg.norm(uq_ref.evaluate(ref.TT(_cores(x)), rv) - sols) / np.linalg.norm(sols)
    print("error %.3e (restatement %.3e), residual %.3e (restatement %.3e)" % (err, oerr, res, ohist[-1]))
    assert err <= 1000 * oerr
    assert res <= 1000 * ohist[-1]


def _cores(x):
    return [x.get_component(k).to_ndarray() for k in range(x.degree())]


@pytest.mark.parametrize("num_special", [0, 1])
def test_uq_mc_and_avg(xe, ref, num_special):
    dims, ranks, N = [6, 3, 4], [3, 2], 100
    t = ref.TT.random(dims, ranks, ref.Rng(17))
    x = _tt_from(xe, t.cores)
    rv, sols = xe.uq_mc(x, N, num_special)
    orv, osols = uq_ref.uq_mc(t, N, num_special)
    assert np.array_equal(np.asarray(rv), orv)            # the stream of Rng(5489) in the reference's order
    got = np.stack([s.to_ndarray() for s in sols])
    assert got.shape == (N, dims[0])
    assert _rel(got, osols) <= 1e-12
    avg = xe.uq_avg(x, N, num_special).to_ndarray()
    assert avg.shape == (dims[0],)
    assert _rel(avg, got.mean(axis=0)) <= 1e-12
    assert np.array_equal(avg, xe.uq_avg(x, N, num_special).to_ndarray())   # fixed-order reduction


def _unit_initial(d, n0, seed):
    init_rv = np.diag(np.arange(1, d, dtype=np.float64))          # unit directions, positive diagonal
    init_sols = np.random.default_rng(seed).standard_normal((d - 1, n0))
    return init_rv, init_sols


def test_measurement_set_with_initial_measurements(xe):
    """uq_adf(UQMeasurementSet, guess) with initial measurements (uqAdf.cpp:338-405): the start is built from
    the mean and the linear terms and rounded at 0.00025 -- looser (1e-7) because of that rounding inside."""
    dims, ranks, N, seed = [6, 3, 4, 3], [4, 4, 2], 257, 7
    _, rv, sols, x0 = uq_ref.make_case(dims, ranks, N, seed)
    init_rv, init_sols = _unit_initial(len(dims), dims[0], seed)
    ox, ohist = uq_ref.uq_adf_measurements(x0, rv, sols, init_rv, init_sols, 6)
    m = xe.UQMeasurementSet()
    for r, s in zip(rv.tolist(), _tensors(xe, sols)):
        m.add(r, s)
    for r, s in zip(init_rv.tolist(), _tensors(xe, init_sols)):
        m.add_initial(r, s)
    assert len(m.randomVectors) == N and len(m.initialSolutions) == len(dims) - 1
    x, hist = xe.uq_adf(m, _tt_from(xe, x0.cores), 6)
    assert x.ranks() == ox.ranks
    assert len(hist) == len(ohist)
    print("set form: history rel dev %.3e, tensor rel dev %.3e" % (np.abs(np.asarray(hist) / np.asarray(ohist) - 1).max(),
                                                                    _rel(_full(xe, x), ox.full())))
    assert np.all(np.abs(np.asarray(hist) - np.asarray(ohist)) <= 1e-7 * np.asarray(ohist))
    assert _rel(_full(xe, x), ox.full()) <= 1e-7
    # a non-unit direction, a non-positive diagonal and a wrong count of initial measurements are refused
    for bad in ([[1.0, 0.5, 0.0]], [[-1.0, 0.0, 0.0]], None):
        mb = xe.UQMeasurementSet(m)
        if bad is None:
            mb.initialRandomVectors = m.initialRandomVectors[:2]
            mb.initialSolutions = m.initialSolutions[:2]
        else:
            mb.initialRandomVectors = bad + m.initialRandomVectors[1:]
        with pytest.raises(Exception):
            xe.uq_adf(mb, _tt_from(xe, x0.cores), 1)


def test_measurement_set_without_initial_equals_plain_call(xe):
    dims, ranks, N, seed = [5, 3, 4], [2, 3], 64, 4
    _, rv, sols, x0 = uq_ref.make_case(dims, ranks, N, seed)
    ts = _tensors(xe, sols)
    m = xe.UQMeasurementSet()
    for r, s in zip(rv.tolist(), ts):
        m.add(r, s)
    guess = _tt_from(xe, x0.cores)
    got = xe.uq_adf(m, guess)
    plain = _tt_from(xe, x0.cores)
    xe.uq_adf(plain, rv.tolist(), ts)
    assert np.array_equal(_full(xe, got), _full(xe, plain))
    assert _rel(_full(xe, guess), x0.full()) <= 1e-14      # the guess is left as it was


def test_preconditions_raise(xe):
    dims, ranks, N, seed = [5, 3, 4], [2, 3], 8, 4
    _, rv, sols, x0 = uq_ref.make_case(dims, ranks, N, seed)
    ts = _tensors(xe, sols)
    x = _tt_from(xe, x0.cores)
    with pytest.raises(Exception, match="random vectors but"):
        xe.uq_adf(x, rv.tolist()[:-1], ts)
    with pytest.raises(Exception, match="entries, expected"):
        xe.uq_adf(x, [r[:1] for r in rv.tolist()], ts)
    with pytest.raises(Exception, match="has size"):
        xe.uq_adf(x, rv.tolist(), _tensors(xe, np.zeros((N, dims[0] + 1))))
    x1 = _tt_from(xe, [np.ones((1, 5, 1))])
    with pytest.raises(Exception, match="degree >= 2"):
        xe.uq_adf(x1, [[] for _ in range(N)], ts)
    m = xe.UQMeasurementSet()
    m.add(rv[0].tolist(), ts[0])
    m.randomVectors = rv.tolist()[:2]
    with pytest.raises(Exception, match="Invalid measurments"):
        xe.uq_adf(m, x)
    # nothing above touched x
    assert _rel(_full(xe, x), x0.full()) <= 1e-14
