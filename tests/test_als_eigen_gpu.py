"""The lowest eigenpair of a TT operator on the GPU: the device-resident LOBPCG on the local GEMM chain
(xrs_als_local_eig) and the ALS_EIGEN sweep, against numpy (tests/als_eigen_ref.py), closed forms and dense
eigenvalues."""
import copy

import numpy as np
import pytest

import als_eigen_ref as er
import als_local_ref as lr

pytestmark = pytest.mark.gpu

TOL = 1e-10
MID = (5, 3, 7, 2, 3)
BIG = (33, 4, 31, 2, 2)


def _upload(handle, p):
    return handle.array(p.L), handle.array(p.A), handle.array(p.R)


# ------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("dims", er.SHAPES)
def test_local_eig_meets_the_bars(handle, dims):
    p = lr.problem(dims, False)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    theta, iters, relres, status = handle.als_local_eig(x, dims, L, A, R, TOL, 0, 16)
    er.check_eigenpair(p, x.numpy(), theta, iters, relres, status, TOL)


@pytest.mark.parametrize("dims", [MID, BIG])
def test_freeze_result_does_not_depend_on_check_every(handle, dims):
    p = lr.problem(dims, False)
    L, A, R = _upload(handle, p)
    runs = []
    max_iter = 200
    for check_every in (1, 7, max_iter):
        x = handle.array(p.x0)
        res = handle.als_local_eig(x, dims, L, A, R, TOL, max_iter, check_every)
        runs.append((x.numpy(), res))
    assert runs[0][1][3] == 0 and runs[0][1][1] < max_iter - 7
    for x, res in runs[1:]:
        assert res == runs[0][1]
        assert np.array_equal(x, runs[0][0])


def test_start_at_the_eigenvector(handle):
    p = lr.problem(MID, False)
    L, A, R = _upload(handle, p)
    w, V = np.linalg.eigh(p.M)
    x = handle.array(V[:, 0].reshape(MID[:3]))
    theta, iters, relres, status = handle.als_local_eig(x, MID, L, A, R, TOL)
    assert (iters, status) == (0, 0) and relres <= TOL
    assert theta == pytest.approx(w[0], rel=1e-13)
    assert np.allclose(x.numpy().reshape(-1), V[:, 0], rtol=0, atol=4 * lr.EPS)   # (normalised again: one rounding)


def test_max_iter_takes_the_restatements_steps(handle):
    p = lr.problem(BIG, False)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    theta, iters, relres, status = handle.als_local_eig(x, BIG, L, A, R, TOL, 3, 16)
    assert (iters, status) == (3, 1)
    want = er.lobpcg(p.matvec, p.x0, TOL, max_iter=3)
    assert np.linalg.norm(x.numpy() - want[0]) <= 1e-10 * np.linalg.norm(want[0])
    assert theta == pytest.approx(want[1], rel=1e-10)
    assert relres == pytest.approx(want[3], rel=1e-8) and relres > TOL


def test_illegal_arguments(handle):
    from xerus_amd import capi

    p = lr.problem(MID, False)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    good = [x, MID, L, A, R, TOL]
    for pos in (0, 2, 3, 4):           # a null pointer
        args = list(good)
        args[pos] = None
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_eig(*args)
        assert info.value.code == -1
    for k in range(5):                 # a zero extent
        zd = tuple(0 if i == k else v for i, v in enumerate(MID))
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_eig(x, zd, L, A, R, TOL)
        assert info.value.code == -1
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_eig(x, MID, L, A, R, tol)
        assert info.value.code == -1
    with pytest.raises(capi.XrsError) as info:   # check_every = 0
        handle.als_local_eig(x, MID, L, A, R, TOL, 0, 0)
    assert info.value.code == -1
    assert handle.lib.xrs_last_error()
    assert np.array_equal(x.numpy(), p.x0)


def test_breakdowns_are_a_status(handle):
    """A NaN operand and a zero start end as XRS_EIG_BREAKDOWN before the first step."""
    p = lr.problem(MID, False)
    L, A, R = _upload(handle, p)
    Lnan = p.L.copy()
    Lnan[1, 0, 2] = np.nan
    x = handle.array(p.x0)
    theta, iters, relres, status = handle.als_local_eig(x, MID, handle.array(Lnan), A, R, TOL, 0, 7)
    assert (iters, status) == (0, 2)
    assert np.isfinite(x.numpy()).all()
    x = handle.zeros(MID[:3])
    theta, iters, relres, status = handle.als_local_eig(x, MID, L, A, R, TOL)
    assert (iters, status) == (0, 2)
    assert not x.numpy().any()


# ------------------------------------------------------------------------------------------- algorithm level
def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _operator(xe, cores):
    A = xe.TTOperator([c.shape[1] for c in cores] + [c.shape[2] for c in cores])
    for k, c in enumerate(cores):
        A.set_component(k, _tensor(xe, c))
    return A


def _tt(xe, cores, core_position=None):
    x = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        x.set_component(k, _tensor(xe, c))
    if core_position is not None:
        x.move_core(core_position, True)
    return x


def _dense(xe, x):
    return xe.Tensor(x).to_ndarray().reshape(-1)


@pytest.mark.parametrize("d,n,ranks", [(4, 4, [2, 3, 2]), (5, 3, [2, 4, 4, 2])])
def test_als_eigen_laplace(xe, d, n, ranks):
    cores = er.laplace_cores(d, n)
    x = _tt(xe, er.random_start([n] * d, ranks, seed=3), core_position=2)
    lam = xe.ALS_EIGEN(_operator(xe, cores), x, 6)
    lam1, lam2, v = er.laplace_lowest(d, n)
    xv = _dense(xe, x)
    res = np.linalg.norm(er.op_dense(cores) @ xv - lam * xv)
    sin = np.linalg.norm(xv - v.reshape(-1) * (v.reshape(-1) @ xv)) / np.linalg.norm(xv)
    print("d %d n %d: lambda error %.1e residual %.1e sin %.1e | ||x|| - 1 | %.1e" %
          (d, n, abs(lam - lam1) / lam1, res, sin, abs(np.linalg.norm(xv) - 1.0)))
    assert abs(lam - lam1) <= 1e-9 * lam1
    assert sin <= 2 * res / (lam2 - lam1)
    assert x.ranks() == ranks
    assert abs(np.linalg.norm(xv) - 1.0) <= 1e-12
    assert x.canonicalized and x.corePosition == 2


def test_als_eigen_full_rank_perturbed(xe):
    cores = er.perturbed_cores(4, 4)
    w = np.linalg.eigvalsh(er.op_dense(cores))
    x = _tt(xe, er.random_start([4] * 4, [4, 16, 4], seed=3))
    lam = xe.ALS_EIGEN(_operator(xe, cores), x, 6)
    print("lambda error %.1e" % (abs(lam - w[0]) / abs(w[0])))
    assert abs(lam - w[0]) <= 1e-9 * abs(w[0])
    assert x.canonicalized and x.ranks() == [4, 16, 4]


def test_als_eigen_low_rank_perturbed(xe):
    """Do not compare tensors with the restatement at low rank (eigenvectors move by residual / gap): lambda only.
    With this start lambda = -31.4634344196 and the restated sweep's eighth half sweep still changes it by 2.2e-9, so
    both runs sit at the fixed point to about 1e-10 relative, inside the 1e-8 bar (measured: equal to 12 digits)."""
    d, n, ranks = 5, 3, [2, 4, 4, 2]
    cores = er.perturbed_cores(d, n)
    M = er.op_dense(cores)
    w = np.linalg.eigvalsh(M)
    norm2 = np.abs(w).max()
    start = er.random_start([n] * d, ranks, seed=3)
    A = _operator(xe, cores)
    x = _tt(xe, start)
    eight = copy.copy(xe.ALS_EIGEN)
    eight.convergenceEpsilon = 0.0   # (all 8 half sweeps, as the restatement with eps = 0: no early end on lambda)
    lam = eight(A, x, 8)
    xv = _dense(xe, x)
    want, _ = er.sweep(cores, start, 8)
    print("lambda %.12f restated %.12f | lambda - <x, A x> | %.1e ||A||" % (lam, want, abs(lam - xv @ M @ xv) / norm2))
    assert abs(lam - xv @ M @ xv) <= 1e-12 * norm2
    assert lam >= w[0] - 1e-12 * norm2
    assert abs(lam - want) <= 1e-8 * abs(want)
    assert x.ranks() == ranks and abs(np.linalg.norm(xv) - 1.0) <= 1e-12
    history = [xe.ALS_EIGEN(A, _tt(xe, start), k) for k in (1, 2, 3, 4)]
    assert all(b <= a + 1e-12 * norm2 for a, b in zip(history, history[1:])), history
    assert lam <= history[-1] + 1e-12 * norm2


def test_fields_and_copies(xe):
    v = xe.ALS_EIGEN
    assert (v.numHalfSweeps, v.convergenceEpsilon, v.preserveCorePosition) == (
        xe.ALS.numHalfSweeps, xe.ALS.convergenceEpsilon, xe.ALS.preserveCorePosition)
    assert v.localTolerance == 1e-10 and v.localMaxIterations == 0
    c = copy.copy(v)
    c.numHalfSweeps, c.convergenceEpsilon, c.preserveCorePosition, c.localTolerance, c.localMaxIterations = 3, 1e-3, False, 1e-6, 9
    assert (c.numHalfSweeps, c.convergenceEpsilon, c.preserveCorePosition, c.localTolerance, c.localMaxIterations) == (3, 1e-3, False, 1e-6, 9)
    assert (v.numHalfSweeps, v.convergenceEpsilon, v.preserveCorePosition, v.localTolerance, v.localMaxIterations) == (0, 1e-6, True, 1e-10, 0)


def test_call_forms_and_core_position(xe):
    d, n, ranks = 4, 4, [2, 3, 2]
    cores = er.laplace_cores(d, n)
    A = _operator(xe, cores)
    start = er.random_start([n] * d, ranks, seed=5)
    lam1 = er.laplace_lowest(d, n)[0]
    x = _tt(xe, start, core_position=1)
    assert xe.ALS_EIGEN(A, x) == pytest.approx(lam1, rel=1e-6)          # the default end rule (epsilon 1e-6)
    assert x.canonicalized and x.corePosition == 1
    x = _tt(xe, start, core_position=1)
    assert xe.ALS_EIGEN(A, x, 1e-9) == pytest.approx(lam1, rel=1e-8)    # an epsilon
    c = copy.copy(xe.ALS_EIGEN)
    c.preserveCorePosition, c.convergenceEpsilon = False, 0.0
    x = _tt(xe, start, core_position=1)
    c(A, x, 3)                                                          # three half sweeps end at the last site
    assert x.canonicalized and x.corePosition == d - 1


def test_iteration_limit_warns_and_goes_on(xe, capfd):
    d, n = 4, 4
    A = _operator(xe, er.laplace_cores(d, n))
    x = _tt(xe, er.random_start([n] * d, [2, 3, 2], seed=3))
    variant = copy.copy(xe.ALS_EIGEN)
    variant.localMaxIterations = 1
    lam = variant(A, x, 2)
    assert np.isfinite(lam) and x.ranks() == [2, 3, 2]
    assert np.isfinite(_dense(xe, x)).all()
    assert "site" in capfd.readouterr().err
    assert xe.ALS_EIGEN.localMaxIterations == 0


def test_mismatched_dimensions_and_breakdown_raise(xe):
    A = _operator(xe, er.laplace_cores(4, 4))
    short, long_ = _tt(xe, er.random_start([4, 4, 3, 4], [2, 3, 2], seed=3)), _tt(xe, er.random_start([4] * 5, [2, 3, 3, 2], seed=3))
    with pytest.raises(xe.generic_error, match="dimension mismatch at mode 2"):
        xe.ALS_EIGEN(A, short, 2)
    with pytest.raises(xe.generic_error, match="degree mismatch"):
        xe.ALS_EIGEN(A, long_, 2)
    cores = er.laplace_cores(4, 4)
    cores[0][0, 1, 2, 1] = np.nan   # (the first local operator is not finite; the right stack does not hold this core)
    with pytest.raises(xe.generic_error, match="site 0"):
        xe.ALS_EIGEN(_operator(xe, cores), _tt(xe, er.random_start([4] * 4, [2, 3, 2], seed=3)), 2)


def test_degree_one(xe):
    n = 6
    rng = np.random.default_rng(4)
    B = rng.standard_normal((n, n))
    B = B + B.T
    x = _tt(xe, [rng.standard_normal((1, n, 1))])
    lam = xe.ALS_EIGEN(_operator(xe, [B.reshape(1, n, n, 1)]), x)
    w, V = np.linalg.eigh(B)
    xv = _dense(xe, x)
    assert abs(lam - w[0]) <= 1e-12 * np.abs(w).max()
    assert np.linalg.norm(B @ xv - lam * xv) <= 2e-10 * np.linalg.norm(B, 2)
    assert abs(np.linalg.norm(xv) - 1.0) <= 1e-12


def test_existing_variants_are_bitwise_unchanged_around_an_eigen_call(xe):
    """ALS_SPD_MF (the CG's scratch regions) and DMRG_SPD, twice around an ALS_EIGEN call: the shared scratch areas
    do not interfere."""
    d, n = 4, 4
    A = _operator(xe, er.laplace_cores(d, n, shift=0.5))
    b = _tt(xe, er.random_start([n] * d, [2, 2, 2], seed=6))
    start = er.random_start([n] * d, [2, 3, 2], seed=7)

    def run(name):
        x = _tt(xe, start)
        energy = getattr(xe, name)(A, x, b, 4)
        return energy, [x.get_component(k).to_ndarray() for k in range(d)]

    before = {name: run(name) for name in ("ALS_SPD_MF", "DMRG_SPD")}
    xe.ALS_EIGEN(A, _tt(xe, start), 2)
    for name, (energy, comps) in before.items():
        again, comps2 = run(name)
        assert again == energy, name
        for a, c in zip(comps, comps2):
            assert np.array_equal(a, c), name
