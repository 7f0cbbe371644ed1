"""Matrix-free ALS on the GPU: the local operator as a GEMM chain (xrs_als_local_apply), the device-resident CG
(xrs_als_local_cg) and the ALS_MF / ALS_SPD_MF variants, against numpy (tests/als_local_ref.py) and the oracle."""
import copy

import numpy as np
import pytest

import als_local_ref as lr

pytestmark = pytest.mark.gpu

CASES = [(dims, normal) for dims in lr.SHAPES for normal in (False, True)]
TOL = 1e-10
BIG = (33, 4, 31, 2, 2)


def _upload(handle, p):
    return handle.array(p.L), handle.array(p.A), handle.array(p.R)


# ------------------------------------------------------------------------------------------- the product
@pytest.mark.parametrize("dims,normal", CASES)
def test_apply_matches_einsum(handle, dims, normal):
    """Elementwise forward bound of the chain: 8 (K_1 + K_2 + ...) eps (|L| |A| |R| |x|), K_i the chain's contraction
    lengths."""
    x, L, A, R = lr.random_operands(dims, normal, seed=3)
    y = handle.empty(dims[:3])
    handle.als_local_apply(y, handle.array(x), dims, handle.array(L), handle.array(A), handle.array(R), normal)
    want = lr.apply_einsum(x, L, A, R, normal)
    bound = 8 * sum(lr.contraction_lengths(dims, normal)) * lr.EPS * lr.apply_einsum(*map(np.abs, (x, L, A, R)), normal)
    err = np.abs(y.numpy() - want)
    assert np.all(err <= bound), float(np.max(err / bound))


# ------------------------------------------------------------------------------------------- CG
@pytest.mark.parametrize("dims,normal", CASES)
def test_cg_solves_the_local_system(handle, dims, normal):
    p = lr.problem(dims, normal)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    iters, relres, status = handle.als_local_cg(x, handle.array(p.b), dims, L, A, R, normal, TOL, 0, 16)
    assert status == 0
    assert 0 < iters <= 4 * p.N + 50
    p.check_solution(x.numpy(), relres, TOL)


@pytest.mark.parametrize("dims,normal", [((5, 3, 7, 2, 3), False), (BIG, False), (BIG, True)])
def test_freeze_result_does_not_depend_on_check_every(handle, dims, normal):
    p = lr.problem(dims, normal)
    L, A, R = _upload(handle, p)
    b = handle.array(p.b)
    runs = []
    max_iter = 120   # (well above the iterations needed: with check_every = max_iter the frozen tail is most of the run)
    for check_every in (1, 7, max_iter):
        x = handle.array(p.x0)
        res = handle.als_local_cg(x, b, dims, L, A, R, normal, TOL, max_iter, check_every)
        runs.append((x.numpy(), res))
    assert runs[0][1][2] == 0 and runs[0][1][0] < max_iter - 7
    for x, res in runs[1:]:
        assert res == runs[0][1]
        assert np.array_equal(x, runs[0][0])


def test_cg_zero_right_hand_side(handle):
    p = lr.problem(BIG, False)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    res = handle.als_local_cg(x, handle.zeros(BIG[:3]), BIG, L, A, R, False, TOL)
    assert res == (0, 0.0, 0)
    assert not x.numpy().any()


@pytest.mark.parametrize("normal", [False, True])
def test_cg_start_at_the_solution(handle, normal):
    dims = (5, 3, 7, 2, 3)
    p = lr.problem(dims, normal)
    L, A, R = _upload(handle, p)
    x = handle.array(p.solution)
    iters, relres, status = handle.als_local_cg(x, handle.array(p.b), dims, L, A, R, normal, TOL)
    assert (iters, status) == (0, 0) and relres <= TOL
    assert np.array_equal(x.numpy(), p.solution)


def test_cg_max_iter(handle):
    p = lr.problem(BIG, False)
    L, A, R = _upload(handle, p)
    x = handle.array(p.x0)
    iters, relres, status = handle.als_local_cg(x, handle.array(p.b), BIG, L, A, R, False, TOL, 3, 16)
    assert (iters, status) == (3, 1)
    assert np.isfinite(x.numpy()).all() and relres > TOL
    # the same three steps as the restatement
    want = lr.cg(p.matvec, p.x0, p.b, TOL, max_iter=3)
    assert np.allclose(x.numpy(), want[0], rtol=1e-12, atol=1e-12 * np.abs(want[0]).max())
    assert relres == pytest.approx(want[2], rel=1e-10)


def test_cg_breakdown_is_a_status(handle):
    """R negated: the operator is negative definite, p^T M p < 0 at the first step; x stays the start."""
    p = lr.problem((5, 3, 7, 2, 3), False)
    dims = p.dims
    x = handle.array(p.x0)
    res = handle.als_local_cg(x, handle.array(p.b), dims, handle.array(p.L), handle.array(p.A), handle.array(-p.R), False, TOL, 0, 7)
    assert res[0] == 0 and res[2] == 2
    assert np.array_equal(x.numpy(), p.x0)
    p = lr.problem(BIG, False)
    x = handle.array(p.x0)
    res = handle.als_local_cg(x, handle.array(p.b), BIG, handle.array(p.L), handle.array(p.A), handle.array(-p.R), False, TOL)
    assert res[2] == 2 and np.isfinite(x.numpy()).all()


def test_illegal_arguments(handle):
    from xerus_amd import capi

    dims = (5, 3, 7, 2, 3)
    p = lr.problem(dims, False)
    L, A, R = _upload(handle, p)
    x, y = handle.array(p.x0), handle.empty(dims[:3])
    good = [y, x, dims, L, A, R, False]
    for pos in (0, 1, 3, 4, 5):   # a null pointer
        args = list(good)
        args[pos] = None
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_apply(*args)
        assert info.value.code == -1
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_cg(*args, TOL)
        assert info.value.code == -1
    for k in range(5):            # a zero extent
        zd = tuple(0 if i == k else v for i, v in enumerate(dims))
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_apply(y, x, zd, L, A, R, False)
        assert info.value.code == -1
        with pytest.raises(capi.XrsError) as info:
            handle.als_local_cg(y, x, zd, L, A, R, False, TOL)
        assert info.value.code == -1
    with pytest.raises(capi.XrsError):   # aliasing
        handle.als_local_apply(x, x, dims, L, A, R, False)
    with pytest.raises(capi.XrsError):
        handle.als_local_cg(x, x, dims, L, A, R, False, TOL)
    with pytest.raises(capi.XrsError):   # check_every = 0
        handle.als_local_cg(y, x, dims, L, A, R, False, TOL, 0, 0)
    assert np.array_equal(x.numpy(), p.x0)


# ------------------------------------------------------------------------------------------- ALS level
def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _laplace_cores(d, n, shift=0.0):
    return [lr.laplace_core(n, 1 if k == 0 else 2, 1 if k == d - 1 else 2, shift) for k in range(d)]


def _operator(xe, cores):
    A = xe.TTOperator([c.shape[1] for c in cores] + [c.shape[2] for c in cores])
    for k, c in enumerate(cores):
        A.set_component(k, _tensor(xe, c))
    return A


def _oracle_tt(ref, tt):
    o = ref.TT([tt.get_component(k).to_ndarray() for k in range(tt.degree())])
    o.canonicalized, o.core_position = tt.canonicalized, tt.corePosition
    return o


@pytest.mark.parametrize("d,n,xr,br", [(4, 4, [2, 3, 2], [2, 2, 2]), (5, 3, [2, 4, 5, 2], [2, 2, 2, 2])])
@pytest.mark.parametrize("variant,spd", [("ALS_SPD_MF", True), ("ALS_MF", False)])
def test_matrix_free_als_matches_oracle(xe, ref, variant, spd, d, n, xr, br):
    """The setup and the bars of test_als_matches_oracle; the oracle solves its local systems directly."""
    rng = np.random.default_rng(11)
    cores = _laplace_cores(d, n, shift=0.0 if spd else 0.3)
    if not spd:
        cores = [c + 0.1 * rng.standard_normal(c.shape) * (c != 0) for c in cores]
    A = _operator(xe, cores)
    b = xe.TTTensor.random([n] * d, br)
    x = xe.TTTensor.random([n] * d, xr)
    ob, ox = _oracle_tt(ref, b), _oracle_tt(ref, x)
    en = getattr(xe, variant)(A, x, b, 6)
    oen = ref.als(cores, ox, ob, spd=spd, num_half_sweeps=6)
    assert x.ranks() == ox.ranks
    assert _rel(xe.Tensor(x).to_ndarray(), ox.full()) <= 1e-9
    assert en == pytest.approx(oen, rel=1e-9, abs=1e-12)
    assert x.canonicalized and x.corePosition == 0


def test_matrix_free_als_spd_reaches_dense_solution(xe, ref):
    """The bar of test_dmrg_spd_reaches_dense_solution."""
    d, n = 4, 4
    cores = _laplace_cores(d, n, shift=0.5)
    A = _operator(xe, cores)
    b = xe.TTTensor.random([n] * d, [2, 2, 2])
    x = xe.TTTensor.random([n] * d, [4, 16, 4])
    xe.ALS_SPD_MF(A, x, b, 1e-13)
    N = n ** d
    M = ref.op_full(cores).reshape(N, N)
    xs = np.linalg.solve(M, xe.Tensor(b).to_ndarray().reshape(N))
    assert _rel(xe.Tensor(x).to_ndarray().reshape(N), xs) <= 1e-9


def test_matrix_free_variants_and_fields(xe):
    assert xe.ALS_MF.matrixFree and xe.ALS_SPD_MF.matrixFree and not xe.ALS.matrixFree and not xe.DMRG_SPD.matrixFree
    assert xe.ALS_SPD_MF.assumeSPD and not xe.ALS_MF.assumeSPD and xe.ALS_MF.sites == 1
    assert xe.ALS_MF.localTolerance == 1e-12 and xe.ALS_MF.localMaxIterations == 0


def test_matrix_free_dmrg_raises(xe):
    d, n = 4, 4
    A = _operator(xe, _laplace_cores(d, n, shift=0.5))
    b = xe.TTTensor.random([n] * d, [2, 2, 2])
    x = xe.TTTensor.random([n] * d, [2, 3, 2])
    variant = copy.copy(xe.DMRG_SPD)
    variant.matrixFree = True
    with pytest.raises(Exception, match="single site"):
        variant(A, x, b, 2)
    assert not xe.DMRG_SPD.matrixFree


def test_matrix_free_indefinite_operator_raises(xe):
    """An indefinite operator given to the SPD variant: the CG's breakdown status becomes an error naming the site."""
    d, n = 4, 4
    cores = _laplace_cores(d, n, shift=0.5)
    cores[0] = -cores[0]
    A = _operator(xe, cores)
    b = xe.TTTensor.random([n] * d, [2, 2, 2])
    x = xe.TTTensor.random([n] * d, [2, 3, 2])
    with pytest.raises(Exception, match="not positive definite"):
        xe.ALS_SPD_MF(A, x, b, 2)


def test_matrix_free_iteration_limit_warns_and_goes_on(xe, capfd):
    """localMaxIterations reached: a warning on stderr per site, as the SVD's non-convergence warns; the sweep goes on."""
    d, n = 4, 4
    A = _operator(xe, _laplace_cores(d, n, shift=0.5))
    b = xe.TTTensor.random([n] * d, [2, 2, 2])
    x = xe.TTTensor.random([n] * d, [2, 3, 2])
    variant = copy.copy(xe.ALS_SPD_MF)
    variant.localMaxIterations = 1
    energy = variant(A, x, b, 2)
    assert np.isfinite(energy) and x.ranks() == [2, 3, 2]
    assert np.isfinite(xe.Tensor(x).to_ndarray()).all()
    assert "CG at site" in capfd.readouterr().err
    assert xe.ALS_SPD_MF.localMaxIterations == 0


def test_matrix_free_without_operator_is_plain_als(xe):
    d, n = 5, 3
    b = xe.TTTensor.random([n] * d, [2, 3, 3, 2])
    x1 = xe.TTTensor.random([n] * d, [2, 2, 2, 2])
    x2 = xe.TTTensor(x1)
    e1 = xe.ALS(x1, b, 4)
    e2 = xe.ALS_MF(x2, b, 4)
    assert e1 == e2
    for k in range(d):
        assert np.array_equal(x1.get_component(k).to_ndarray(), x2.get_component(k).to_ndarray())
