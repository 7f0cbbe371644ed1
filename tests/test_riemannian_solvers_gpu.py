"""SteepestDescentVariant and GeometricCGVariant on the GPU against the NumPy restatement of the reference's
loops (tests/riemannian_ref.py; steepestDescent.cpp:37-176, cg.cpp:38-124).

Problem: modes [4, 4, 4, 4], ranks [2, 3, 2], numpy.random.default_rng(3): b is drawn first, then x0, which is
moved to core 0. The restatement starts from the cores of x0 read back from the GPU; residuals are gauge
invariant. Checked on the CPU with the restatement (a 1e-13 relative perturbation of the cores of x0):
  - steepest descent with SubmanifoldRetractionII reaches 1e-8 (1e-10 ||b||) at step 9; the perturbation moves
    the residuals of steps 1-8 by at most 3e-11 relative, so that prefix is well defined;
  - geometric CG (no operator, and the shifted Laplace operator with both values of
    assumeSymmetricPositiveDefiniteOperator): the perturbation moves none of the first 16 residuals by more than
    2e-13 relative, far below 1e-8: K = 16, the whole run of 16 steps.
"""
import numpy as np
import pytest

import riemannian_ref as rr

pytestmark = pytest.mark.gpu

DIMS, RANKS = [4, 4, 4, 4], [2, 3, 2]
CG_STEPS = 16   # = K, see the module docstring


def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _random_cores(rng, dims, ranks):
    r = [1] + list(ranks) + [1]
    return [rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))]


def _tt(xe, cores):
    t = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        t.set_component(k, _tensor(xe, c))
    return t


def _oracle(ref, tt):
    o = ref.TT([tt.get_component(k).to_ndarray() for k in range(tt.degree())])
    o.canonicalized, o.core_position = tt.canonicalized, tt.corePosition
    return o


def _laplace_cores(d, n, shift):   # the operator of test_als_gpu.py
    L = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1) + shift * np.eye(n)
    I = np.eye(n)
    cs = []
    for k in range(d):
        if k == 0:
            c = np.zeros((1, n, n, 2)); c[0, :, :, 0] = L; c[0, :, :, 1] = I
        elif k == d - 1:
            c = np.zeros((2, n, n, 1)); c[0, :, :, 0] = I; c[1, :, :, 0] = L
        else:
            c = np.zeros((2, n, n, 2)); c[0, :, :, 0] = I; c[1, :, :, 0] = L; c[1, :, :, 1] = I
        cs.append(c)
    return cs


def _operator(xe, cores):
    A = xe.TTOperator([c.shape[1] for c in cores] + [c.shape[2] for c in cores])
    for k, c in enumerate(cores):
        A.set_component(k, _tensor(xe, c))
    return A


@pytest.fixture(scope="module")
def problem(xe, ref):
    rng = np.random.default_rng(3)
    bcores = _random_cores(rng, DIMS, RANKS)
    b = _tt(xe, bcores)
    x0 = _tt(xe, _random_cores(rng, DIMS, RANKS))
    x0.move_core(0)
    return dict(b=b, x0=x0, ob=ref.TT(bcores), ox0=_oracle(ref, x0), normb=float(np.linalg.norm(ref.TT(bcores).full())))


def test_steepest_descent_follows_the_restatement(xe, problem):
    p = problem
    want = rr.steepest_descent(None, p["ox0"].copy(), p["ob"], 12, 1e-8, rr.submanifold_retraction)
    got = []
    for steps in range(1, 9):   # a run of `steps` steps from x0 returns the residual after step `steps`
        x = xe.TTTensor(p["x0"])
        got.append(xe.SteepestDescent(x, p["b"], steps))
        assert x.ranks() == RANKS
    for k, (g, w) in enumerate(zip(got, want[1:9])):
        print(f"step {k + 1}: residual {g:.12e} (restatement {w:.12e})")
        assert abs(g - w) <= 1e-6 * w
    x = xe.TTTensor(p["x0"])
    final = xe.SteepestDescent(x, p["b"], 12)
    assert final <= 1e-6 * p["normb"]
    assert xe.frob_norm(p["b"] - x) == pytest.approx(final, abs=1e-9 * p["normb"])


@pytest.mark.parametrize("name", ["HOSVDRetraction(3)", "ALSRetractionII"])
def test_steepest_descent_with_other_retractions(xe, problem, name):
    """Residuals never increase, and the run ends within a factor 10 of the restatement with the same
    retraction and the same number of steps (here both converge in two steps: b has the ranks of x)."""
    p = problem
    retraction = xe.HOSVDRetraction(3) if name == "HOSVDRetraction(3)" else xe.ALSRetractionII
    restated = rr.hosvd_retraction(3) if name == "HOSVDRetraction(3)" else rr.als_retraction
    steps = 4
    want = rr.steepest_descent(None, p["ox0"].copy(), p["ob"], steps, 1e-8, restated)
    solver = xe.SteepestDescentVariant(0, 1e-8, False, retraction)
    got = [xe.frob_norm(p["b"] - p["x0"])]
    for k in range(1, len(want)):
        x = xe.TTTensor(p["x0"])
        got.append(solver(x, p["b"], k))
    print(f"{name}: residuals {got} (restatement {want})")
    assert all(b2 <= a2 for a2, b2 in zip(got, got[1:]))
    assert got[-1] <= 10 * want[-1]


CG_CASES = [("none", False), ("laplace", True), ("laplace", False)]


@pytest.mark.parametrize("operator,spd", CG_CASES)
def test_geometric_cg_follows_the_restatement(xe, problem, operator, spd):
    """The retraction is the bound SubmanifoldRetractionI, the transport a Python callable around the bound
    ProjectiveVectorTransport that also records the residual of the point it is given: one entry per step."""
    p = problem
    cores = _laplace_cores(4, 4, 0.3) if operator == "laplace" else None
    A = _operator(xe, cores) if cores is not None else None
    i, j = xe.indices(2)
    trace = []

    def residual(x):
        if A is None:
            return xe.frob_norm(p["b"] - x)
        Ax = xe.TTTensor()
        Ax(i & 0) << A(i / 2, j / 2) * x(j & 0)
        return xe.frob_norm(p["b"] - Ax)

    def transport(new_base, vector):
        trace.append(residual(new_base))
        xe.ProjectiveVectorTransport(new_base, vector)

    solver = xe.GeometricCGVariant(CG_STEPS, 1e-8, spd, xe.SubmanifoldRetractionI, transport)
    x = xe.TTTensor(p["x0"])
    final = solver(x, p["b"], CG_STEPS) if A is None else solver(A, x, p["b"], CG_STEPS)
    ox = p["ox0"].copy()
    want = rr.geometric_cg(cores, ox, p["ob"], CG_STEPS, 1e-8, spd=spd)
    assert len(trace) == CG_STEPS == len(want) - 1
    for k, (g, w) in enumerate(zip(trace, want[1:])):
        print(f"step {k + 1}: residual {g:.12e} (restatement {w:.12e})")
        assert abs(g - w) <= 1e-8 * w
    assert final == pytest.approx(trace[-1], rel=1e-12)
    assert final / p["normb"] <= 10 * want[-1] / p["normb"]
    assert x.ranks() == RANKS and x.canonicalized and x.corePosition == 0


def test_predefined_variants_and_python_retraction(xe, problem):
    """GeometricCG and SteepestDescent carry the reference's defaults; a Python callable is accepted as a
    retraction and updates the solver's point in place."""
    assert xe.SteepestDescent.numSteps == 0 and xe.SteepestDescent.convergenceEpsilon == 1e-8
    assert not xe.SteepestDescent.assumeSymmetricPositiveDefiniteOperator
    assert xe.GeometricCG.numSteps == 0 and xe.GeometricCG.convergenceEpsilon == 1e-8
    p = problem
    calls = []

    def retraction(x, change):
        calls.append(change.frob_norm())
        xe.SubmanifoldRetractionII(x, change)

    x = xe.TTTensor(p["x0"])
    got = xe.SteepestDescentVariant(retraction)(x, p["b"], 3)
    y = xe.TTTensor(p["x0"])
    assert got == pytest.approx(xe.SteepestDescent(y, p["b"], 3), rel=1e-12)
    assert len(calls) >= 3


def test_require_failures_raise(xe, problem):
    p = problem
    rng = np.random.default_rng(4)
    off_core = xe.TTTensor(p["x0"])
    off_core.move_core(1)
    with pytest.raises(xe.generic_error, match="core position 0"):
        xe.TTTangentVector(off_core, p["b"])
    not_canonical = _tt(xe, _random_cores(rng, DIMS, RANKS))
    with pytest.raises(xe.generic_error, match="core position 0"):
        xe.TTTangentVector(not_canonical, p["b"])
    other = _tt(xe, _random_cores(rng, [4, 4, 3, 4], RANKS))
    with pytest.raises(xe.generic_error):
        xe.TTTangentVector(p["x0"], other)
    a = xe.TTTangentVector(p["x0"], p["b"])
    short = _tt(xe, _random_cores(rng, [4, 4, 4], [2, 2]))
    short.move_core(0)
    c = xe.TTTangentVector(short, short)
    with pytest.raises(xe.generic_error):
        a += c
    with pytest.raises(xe.generic_error):
        a.scalar_product(c)
    with pytest.raises(xe.generic_error, match="core position 0"):
        xe.ProjectiveVectorTransport(off_core, a)
