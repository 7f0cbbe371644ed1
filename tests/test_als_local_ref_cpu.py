"""CPU: the numpy restatement of the matrix-free ALS local problem (tests/als_local_ref.py) -- both GEMM chains equal
the defining einsum, the CG with its freeze semantics meets the bars the GPU tests set -- and the new entry points are
declared, bound and exported."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import als_local_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL_SYMBOLS = ["xrs_als_local_apply", "xrs_als_local_cg"]
CASES = [(dims, normal) for dims in lr.SHAPES for normal in (False, True)]
TOL = 1e-10


@pytest.mark.parametrize("dims,normal", CASES)
def test_chain_equals_einsum(dims, normal):
    x, L, A, R = lr.random_operands(dims, normal, seed=3)
    want = lr.apply_einsum(x, L, A, R, normal)
    got = lr.apply_chain(x, L, A, R, normal)
    bound = 8 * sum(lr.contraction_lengths(dims, normal)) * lr.EPS * lr.apply_einsum(*map(np.abs, (x, L, A, R)), normal)
    assert got.shape == want.shape == dims[:3]
    assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))


@pytest.mark.parametrize("dims,normal", CASES)
def test_dense_operator_is_the_product_and_spd(dims, normal):
    p = lr.problem(dims, normal)
    v = np.random.default_rng(1).standard_normal(dims[:3])
    assert np.allclose(p.M @ v.reshape(p.N), p.matvec(v).reshape(p.N), rtol=1e-12, atol=1e-12 * np.abs(p.M).sum(axis=1).max())
    assert np.abs(p.M - p.M.T).max() <= 1e-12 * np.abs(p.M).max()
    assert p.eigenvalues[0] > 0, p.eigenvalues[0]


@pytest.mark.parametrize("dims,normal", CASES)
def test_cg_meets_the_bars(dims, normal):
    p = lr.problem(dims, normal)
    x, iters, relres, status = lr.cg(p.matvec, p.x0, p.b, TOL)
    assert status == lr.CONVERGED
    assert 0 < iters <= 4 * p.N + 50
    p.check_solution(x, relres, TOL)


@pytest.mark.parametrize("dims,normal", [((5, 3, 7, 2, 3), False), ((33, 4, 31, 2, 2), True)])
def test_freeze_makes_the_result_independent_of_check_every(dims, normal):
    p = lr.problem(dims, normal)
    max_iter = 120   # (well above the iterations needed: the frozen tail is most of the run)
    runs = [lr.cg(p.matvec, p.x0, p.b, TOL, max_iter, ce) for ce in (1, 7, max_iter)]
    assert runs[0][3] == lr.CONVERGED and runs[0][1] < max_iter - 7
    for x, iters, relres, status in runs[1:]:
        assert np.array_equal(x, runs[0][0]) and (iters, relres, status) == runs[0][1:]


def test_cg_edge_cases():
    p = lr.problem((33, 4, 31, 2, 2), False)
    x, iters, relres, status = lr.cg(p.matvec, p.x0, np.zeros_like(p.b), TOL)
    assert not x.any() and (iters, relres, status) == (0, 0.0, lr.CONVERGED)
    x, iters, relres, status = lr.cg(p.matvec, p.solution, p.b, TOL)
    assert iters == 0 and status == lr.CONVERGED and np.array_equal(x, p.solution)
    x, iters, relres, status = lr.cg(p.matvec, p.x0, p.b, TOL, max_iter=3)
    assert (iters, status) == (3, lr.MAX_ITER) and np.isfinite(x).all() and relres > TOL
    neg = lambda v: lr.apply_chain(v, p.L, p.A, -p.R, False)  # noqa: E731
    x, iters, relres, status = lr.cg(neg, p.x0, p.b, TOL)
    assert (iters, status) == (0, lr.BREAKDOWN) and np.array_equal(x, p.x0)


def test_environments_are_those_of_the_oracle(ref):
    """The local operator and energy built from environments() equal the oracle's own one-site quantities: the dense
    operator applied to the middle core gives <x, A x> (or <A x, A x>) of the full tensors."""
    for normal in (False, True):
        p = lr.problem((5, 3, 7, 2, 3), normal)
        full_x = ref.TT(p.x_cores).full().reshape(-1)
        Aop = ref.op_full(p.op_cores).reshape(full_x.size, full_x.size)
        want = full_x @ (Aop.T @ (Aop @ full_x)) if normal else full_x @ (Aop @ full_x)
        got = np.sum(p.x0 * p.matvec(p.x0))
        assert got == pytest.approx(want, rel=1e-12)


def test_local_symbols_are_declared_bound_and_exported():
    from xerus_amd import capi

    hdr = open(os.path.join(ROOT, "include", "xerus_amd.h")).read()
    capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (xrs_[a-z0-9_]+)", out))
    for name in LOCAL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SIGNATURES, name
        assert name in exported, name
    assert callable(capi.Handle.als_local_apply) and callable(capi.Handle.als_local_cg)
    for name in ("XRS_CG_CONVERGED 0", "XRS_CG_MAX_ITER 1", "XRS_CG_BREAKDOWN 2"):
        assert "#define " + name in hdr, name


def test_header_compiles_as_c():
    src = ('#include "xerus_amd.h"\n'
           "int use(xrs_handle_t h, double* y, const double* x, const double* e, size_t* it, double* rel, int* st) {\n"
           "    return xrs_als_local_apply(h, y, x, 1, 2, 3, 4, 5, e, e, e, 0) +\n"
           "           xrs_als_local_cg(h, y, x, 1, 2, 3, 4, 5, e, e, e, 1, 1e-10, 0, 1, it, rel, st) + XRS_CG_BREAKDOWN;\n"
           "}\n")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "use.c")
        with open(path, "w") as f:
            f.write(src)
        res = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), path],
                             capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_extents_are_range_checked_before_ctypes_wraps_them():
    from xerus_amd import capi

    with pytest.raises(capi.XrsError) as info:
        capi.Handle._local_extents("xrs_als_local_apply", (1, -2, 3, 4, 5))
    assert info.value.code == -1
    with pytest.raises(capi.XrsError):
        capi.Handle._local_extents("xrs_als_local_cg", (1, 2, 3, 4, 5), max_iter=-1)
    assert capi.Handle._local_extents("xrs_als_local_cg", (1, 2, 3, 4, 5), 0, 7) == (1, 2, 3, 4, 5)
