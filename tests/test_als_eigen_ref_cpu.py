"""CPU: the numpy restatement of the matrix-free eigen sweep (tests/als_eigen_ref.py) meets the bars the GPU tests set
-- the LOBPCG iteration with its freeze semantics and statuses, the sweep against closed forms and dense eigenvalues
-- the host-only 3 x 3 routine of the library (xrs_geneig_lowest) follows its pivot rule, and the new entry points are
declared, bound and exported."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import als_eigen_ref as er
import als_local_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_SYMBOLS = ["xrs_als_local_eig", "xrs_geneig_lowest"]
TOL = 1e-10
MID = (5, 3, 7, 2, 3)
BIG = (33, 4, 31, 2, 2)
# iterations at 1e-10. The tiny extents are a property of the method (N = 1, 2, 3 need 0, 1, 2 steps) and are asserted
# exactly; the others are the counts of the CPU prototype of this iteration, which the restatement reproduces, and are
# asserted within one step (a residual that lands beside the threshold may cross it one step earlier or later under
# another summation order), so that a change that slows the iteration down does not pass unnoticed.
TINY_ITERS = {(1, 1, 1, 1, 1): 0, (1, 2, 1, 1, 1): 1, (1, 3, 1, 2, 1): 2}
PROTOTYPE_ITERS = {(1, 3, 2, 1, 2): 13, (7, 4, 1, 3, 1): 37, (5, 3, 7, 2, 3): 50, (16, 5, 16, 1, 1): 409, (33, 4, 31, 2, 2): 125}


# ------------------------------------------------------------------------------------------- the iteration
@pytest.mark.parametrize("dims", er.SHAPES)
def test_restated_iteration_meets_the_bars(dims):
    p = lr.problem(dims, False)
    info = {}
    x, theta, iters, relres, status = er.lobpcg(p.matvec, p.x0, TOL, info=info)
    er.check_eigenpair(p, x, theta, iters, relres, status, TOL)
    assert info["drops"] == 0   # (the drop branch is the small routine's own test's business)
    if dims in TINY_ITERS:
        assert iters == TINY_ITERS[dims]
    if dims in PROTOTYPE_ITERS:
        assert abs(iters - PROTOTYPE_ITERS[dims]) <= 1, (iters, PROTOTYPE_ITERS[dims])


def test_freeze_makes_the_result_independent_of_check_every():
    p = lr.problem(MID, False)
    max_iter = 200
    runs = [er.lobpcg(p.matvec, p.x0, TOL, max_iter, ce) for ce in (1, 7, max_iter)]
    assert runs[0][4] == er.CONVERGED and runs[0][2] < max_iter - 7
    for run in runs[1:]:
        assert np.array_equal(run[0], runs[0][0]) and run[1:] == runs[0][1:]


def test_iteration_edge_cases():
    p = lr.problem(MID, False)
    w, V = np.linalg.eigh(p.M)
    x, theta, iters, relres, status = er.lobpcg(p.matvec, V[:, 0].reshape(MID[:3]), TOL)
    assert (iters, status) == (0, er.CONVERGED) and theta == pytest.approx(w[0], rel=1e-13)
    p = lr.problem(BIG, False)
    x, theta, iters, relres, status = er.lobpcg(p.matvec, p.x0, TOL, max_iter=3)
    assert (iters, status) == (3, er.MAX_ITER) and np.isfinite(x).all() and relres > TOL
    Lnan = p.L.copy()
    Lnan[1, 0, 2] = np.nan
    x, theta, iters, relres, status = er.lobpcg(lambda v: lr.apply_chain(v, Lnan, p.A, p.R, False), p.x0, TOL)
    assert (iters, status) == (0, er.BREAKDOWN)
    x, theta, iters, relres, status = er.lobpcg(p.matvec, np.zeros_like(p.x0), TOL)
    assert (iters, status) == (0, er.BREAKDOWN) and not x.any()


# ------------------------------------------------------------------------------------------- the small problem
def _pencil(S, M):
    G, H = S.T @ S, S.T @ M @ S
    iu = np.triu_indices(S.shape[1])
    return G[iu], H[iu]


def _dense_lowest(S, M):
    """The smallest pair of the pencil by an orthonormal basis of span(S): (theta, the unit Ritz vector in R^m)."""
    Q = np.linalg.qr(S)[0]
    w, Y = np.linalg.eigh(Q.T @ M @ Q)
    return w[0], Q @ Y[:, 0]


def _sym(rng, m):
    B = rng.standard_normal((m, m))
    return B + B.T


@pytest.mark.parametrize("k", [3, 2])
def test_geneig_lowest_well_conditioned(k):
    from xerus_amd import capi

    rng = np.random.default_rng(7)
    M, S = _sym(rng, 9), rng.standard_normal((9, k)) * np.array([1.0, 1e-3, 50.0])[:k]   # (badly scaled columns)
    G, H = _pencil(S, M)
    used, theta, c = capi.geneig_lowest(k, G, H)
    want_theta, want_v = _dense_lowest(S, M)
    v = S @ c
    assert used == k and c[0] >= 0.0
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-13
    assert abs(theta - want_theta) <= 1e-13 * np.linalg.norm(M, 2)
    assert min(np.linalg.norm(v - want_v), np.linalg.norm(v + want_v)) <= 1e-13
    rused, rtheta, rc = er.geneig_lowest(k, G, H)
    assert rused == used and rtheta == pytest.approx(theta, rel=1e-14) and np.allclose(rc[:k], c, rtol=1e-13, atol=1e-15)


def test_geneig_lowest_drops_a_dependent_third_vector():
    from xerus_amd import capi

    rng = np.random.default_rng(8)
    M, S = _sym(rng, 9), rng.standard_normal((9, 3))
    S[:, 2] = S[:, 1] * (1.0 + 1e-12 * rng.standard_normal(9))
    G, H = _pencil(S, M)
    used, theta, c = capi.geneig_lowest(3, G, H)
    want_theta, want_v = _dense_lowest(S[:, :2], M)
    assert used == 2 and c[2] == 0.0
    assert abs(theta - want_theta) <= 1e-13 * np.linalg.norm(M, 2)
    used2, theta2, c2 = capi.geneig_lowest(2, G[[0, 1, 3]], H[[0, 1, 3]])
    assert (used2, theta2) == (2, theta) and np.array_equal(c2, c[:2])
    assert er.geneig_lowest(3, G, H)[0] == 2


def test_geneig_lowest_breakdowns():
    from xerus_amd import capi

    rng = np.random.default_rng(9)
    M, s = _sym(rng, 9), rng.standard_normal(9)
    S = np.stack([s, s * (1.0 + 1e-12), s * (1.0 - 1e-12)], axis=1)
    G, H = _pencil(S, M)
    assert capi.geneig_lowest(3, G, H)[0] == 0 and er.geneig_lowest(3, G, H)[0] == 0
    assert capi.geneig_lowest(2, G[[0, 1, 3]], H[[0, 1, 3]])[0] == 0
    G, H = _pencil(rng.standard_normal((9, 3)), M)
    bad = H.copy()
    bad[4] = np.nan
    assert capi.geneig_lowest(3, G, bad)[0] == 0 and er.geneig_lowest(3, G, bad)[0] == 0
    zero = G.copy()
    zero[0] = 0.0
    assert capi.geneig_lowest(3, zero, H)[0] == 0
    with pytest.raises(capi.XrsError):
        capi.geneig_lowest(4, G, H)


# ------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("d,n,ranks", [(4, 4, [2, 3, 2]), (5, 3, [2, 4, 4, 2])])
def test_restated_sweep_laplace(d, n, ranks):
    lam, cores = er.sweep(er.laplace_cores(d, n), er.random_start([n] * d, ranks, seed=3), 6)
    want = d * (2.0 - 2.0 * np.cos(np.pi / (n + 1)))
    print("d %d n %d: lambda error %.1e" % (d, n, abs(lam - want) / want))
    assert abs(lam - want) <= 1e-9 * want
    assert er.laplace_lowest(d, n)[0] == pytest.approx(want, rel=1e-15)
    assert [c.shape[2] for c in cores[:-1]] == ranks


def test_restated_sweep_full_rank_perturbed():
    cores = er.perturbed_cores(4, 4)
    M = er.op_dense(cores)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    w = np.linalg.eigvalsh(M)
    lam, _ = er.sweep(cores, er.random_start([4] * 4, [4, 16, 4], seed=3), 6)
    print("lambda error %.1e" % (abs(lam - w[0]) / abs(w[0])))
    assert abs(lam - w[0]) <= 1e-9 * abs(w[0])


def test_restated_sweep_low_rank_is_monotone_and_above_the_spectrum():
    cores = er.perturbed_cores(5, 3)
    M = er.op_dense(cores)
    w = np.linalg.eigvalsh(M)
    norm2 = np.abs(w).max()
    history = []
    lam, xc = er.sweep(cores, er.random_start([3] * 5, [2, 4, 4, 2], seed=3), 8, history=history)
    x = er.tt_dense(xc).reshape(-1)
    assert abs(np.linalg.norm(x) - 1.0) <= 1e-12
    assert abs(lam - x @ M @ x) <= 1e-12 * norm2
    assert lam >= w[0] - 1e-12 * norm2
    assert all(b <= a + 1e-12 * norm2 for a, b in zip(history, history[1:])), history


# ------------------------------------------------------------------------------------------- ABI bookkeeping
def test_eig_symbols_are_declared_bound_and_exported():
    from xerus_amd import capi

    hdr = open(os.path.join(ROOT, "include", "xerus_amd.h")).read()
    capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (xrs_[a-z0-9_]+)", out))
    for name in EIG_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SIGNATURES, name
        assert name in exported, name
    assert callable(capi.Handle.als_local_eig) and callable(capi.geneig_lowest)
    for name in ("XRS_EIG_CONVERGED 0", "XRS_EIG_MAX_ITER 1", "XRS_EIG_BREAKDOWN 2"):
        assert "#define " + name in hdr, name


def test_header_compiles_as_c():
    src = ('#include "xerus_amd.h"\n'
           "int use(xrs_handle_t h, double* x, const double* e, double* th, size_t* it, double* rel, int* st) {\n"
           "    return xrs_als_local_eig(h, x, 1, 2, 3, 4, 5, e, e, e, 1e-10, 0, 1, th, it, rel, st) +\n"
           "           xrs_geneig_lowest(3, e, e, th, x) + XRS_EIG_BREAKDOWN;\n"
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
        capi.Handle._local_extents("xrs_als_local_eig", (1, -2, 3, 4, 5))
    assert info.value.code == -1
    with pytest.raises(capi.XrsError):
        capi.Handle._local_extents("xrs_als_local_eig", (1, 2, 3, 4, 5), check_every=-1)
    assert capi.Handle._local_extents("xrs_als_local_eig", (1, 2, 3, 4, 5), 0, 7) == (1, 2, 3, 4, 5)
