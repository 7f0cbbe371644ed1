"""Dense and TT kernels at the ends of the double range, against the LAPACK-call oracle.

Every factorisation here squares the entries (CholeskyQR on A^T A, Gram eigenproblems, Jacobi row dots, sums
of x^2); the reference calls dgeqp3 / dgesdd / dnrm2, which work at any representable scale. So each routine
is run on A 2^e for exact powers of two, applied with np.ldexp: A 2^e is exact, and the factorisation must
agree with the oracle's of the unscaled A, rescaled by 2^e, at the bars the routine's own tests assert at
scale 1 (tests/test_factorisations_gpu.py, test_svd_bidiag_gpu.py, test_syev_gpu.py, test_als_gpu.py,
test_kernels_gpu.py, test_tt_gpu.py) -- scaling by a power of two must not cost accuracy. Each case also runs
the oracle on the scaled input (the reference copes), and every residual is formed on operands brought back
to O(1) with np.ldexp, so the test's own arithmetic neither overflows nor underflows; norms of raw scaled
data go through dnrm2.

Scales: 2^+-400 (~1e+-120, squares still representable: a guard), 2^+-600 (~1e+-180, squares overflow /
underflow), 2^+-830 (~1e+-250), and for the SVD and the norms 2^-1040 (max |A| subnormal). At 2^-1040 the
input is the rounded np.ldexp(A, -1040) and "unscaled" means that input brought back to O(1) (exact). The
outputs are themselves subnormal there and carry fewer digits, so the bar is max(normal bar, 8 x the oracle's
own deviation on the same input from its unscaled result times 2^e), the factor 8 covering a different but
equally valid operation order. Oracle deviations measured at 2^-1040 (CPU, scipy-openblas): singular values
2.4e-13 .. 4.7e-12 S_0 (random and rank 7), 1.4e-11 (twin); U S Vt residual 6.7e-13 .. 5.5e-12, 1.1e-11
(twin); dnrm2 0 .. 1.6e-12 relative, dasum 0 (sums of subnormals are exact): the quantum 2^-1074 against
entries of 2^-1040.
"""
import numpy as np
import pytest
from scipy.linalg import eigh
from scipy.linalg.blas import dasum, dnrm2

from xerus_amd import capi

pytestmark = pytest.mark.gpu

TOL = 1e-12
SCALES = [0, 400, -400, 600, -600, 830, -830]
SUB = -1040   # max |A| subnormal

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _fro(a):
    """Frobenius norm by the scaled dnrm2 (never squares an entry unscaled)."""
    return float(dnrm2(np.ascontiguousarray(a, dtype=np.float64).ravel()))


def _rel(a, b):
    return _fro(a - b) / max(_fro(b), 1e-300)


def _unscaled(A0, e):
    """(A, A1): the input A = A0 2^e as the kernel gets it and the same matrix brought back to O(1); A1 is A0
    itself unless 2^e pushes entries into the subnormal range, where A is rounded and A1 2^e = A still exact."""
    A = np.ldexp(A0, e)
    A1 = np.ldexp(A, -e)
    assert np.array_equal(np.ldexp(A1, e), A)
    return A, A1


def _finite(*arrays):
    return all(np.all(np.isfinite(a)) for a in arrays)


# ------------------------------------------------------------------------------------------------ SVD
def _orthogonal_pair(rng, n):
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return U, V


def _svd_input(kind, m, n):
    rng = np.random.default_rng(1000 * m + n)
    if kind == "random":
        return rng.standard_normal((m, n))
    assert m == n == 96
    rng = np.random.default_rng(3)
    if kind == "rank7":
        return rng.standard_normal((n, 7)) @ rng.standard_normal((7, n))
    U, V = _orthogonal_pair(rng, n)   # "twin": the pairs of test_svd_square_fallback_cases
    return (U * np.repeat(np.linspace(1, 2, n // 2), 2)) @ V.T


def _check_svd(handle, ref, kind, m, n, e):
    A0 = _cached(("svd", kind, m, n), lambda: _svd_input(kind, m, n))
    A, A1 = _unscaled(A0, e)
    k = min(m, n)
    big = k > 512
    s_bar, res_bar, orth_bar = 1e-12, (1e-13 if big else 1e-14), (1e-12 if big else 1e-14)
    # the oracle on the unscaled matrix, and on the scaled one (brought back): the reference copes
    Sr = _cached(("svd-s", kind, m, n, e if e == SUB else 0), lambda: ref.svd(A1)[1])
    Uo, So, Vo = ref.svd(A)
    So1 = np.ldexp(So, -e)
    assert _finite(Uo, So, Vo)
    dev_s = np.abs(So1 - Sr).max() / Sr[0]
    dev_res = _rel((Uo * So1) @ Vo, A1)
    print(f"svd {kind} {m}x{n} e={e}: oracle deviation S {dev_s:.2e} residual {dev_res:.2e}")
    if e == SUB:
        s_bar, res_bar = max(s_bar, 8 * dev_s), max(res_bar, 8 * dev_res)
    else:
        assert dev_s <= s_bar and dev_res <= res_bar
    Uh, Sh, Vh = (x.numpy() for x in handle.svd(handle.array(A)))
    assert _finite(Uh, Sh, Vh)
    S1 = np.ldexp(Sh, -e)
    err_s = np.abs(S1 - Sr).max() / Sr[0]
    res = _rel((Uh * S1) @ Vh, A1)
    ou, ov = np.abs(Uh.T @ Uh - np.eye(k)).max(), np.abs(Vh @ Vh.T - np.eye(k)).max()
    print(f"svd {kind} {m}x{n} e={e}: S {err_s:.2e} residual {res:.2e} orthogonality {ou:.2e} {ov:.2e}")
    assert np.all(np.diff(Sh) <= 0)
    assert err_s <= s_bar
    assert res <= res_bar
    assert ou <= orth_bar and ov <= orth_bar
    if not big:
        assert np.linalg.norm(Uh.T @ Uh - np.eye(k)) <= TOL * k
        assert np.linalg.norm(Vh @ Vh.T - np.eye(k)) <= TOL * k


# (8,8): n < 16, Jacobi on the rows; (16,16), (96,96): square bidiagonal; (129,129): square Jacobi; (12,200): wide,
# rows directly; (200,12): tall QR then Jacobi; (40,300), (300,40): bidiagonal on the QR factor
SVD_SHAPES = [(8, 8), (16, 16), (96, 96), (129, 129), (12, 200), (200, 12), (40, 300), (300, 40)]


@pytest.mark.parametrize("e", SCALES + [SUB])
@pytest.mark.parametrize("m,n", SVD_SHAPES)
def test_svd_random(handle, ref, m, n, e):
    _check_svd(handle, ref, "random", m, n, e)


@pytest.mark.parametrize("e", [600, -600])
@pytest.mark.parametrize("m,n", [(520, 513), (513, 520)])
def test_svd_above_512(handle, ref, m, n, e):
    """svd_big: CholeskyQR of A, block Jacobi on the triangular factor."""
    _check_svd(handle, ref, "random", m, n, e)


@pytest.mark.parametrize("e", SCALES + [SUB])
@pytest.mark.parametrize("kind", ["rank7", "twin"])
def test_svd_bidiagonal_check_fails(handle, ref, kind, e):
    """96 x 96 spectra the bidiagonal route hands to its fallback (rank 7: zero cluster; twin: pairs), which
    is the range-scaling path of svd()."""
    _check_svd(handle, ref, kind, 96, 96, e)


# ------------------------------------------------------------------------------------------------ QR / RQ
# (8,5), (5,8): small_problem; (300,40), (40,300): orthogonalize below 512; (700,513), (513,700): orthogonalize_big
QR_CASES = [(m, n, e) for (m, n) in [(8, 5), (5, 8), (300, 40), (40, 300)] for e in SCALES] + \
           [(m, n, e) for (m, n) in [(700, 513), (513, 700)] for e in (600, -600)]


def _orth_ok(G, k, big):
    """Q^T Q - I at the bars of test_qr_rq / test_qr_rq_above_512."""
    if big:
        return np.abs(G - np.eye(k)).max() <= 1e-13
    return np.linalg.norm(G - np.eye(k)) <= TOL * k


@pytest.mark.parametrize("m,n,e", QR_CASES)
def test_qr_rq(handle, ref, m, n, e):
    A0 = _cached(("qr", m, n), lambda: np.random.default_rng(m + 3 * n).standard_normal((m, n)))
    A = np.ldexp(A0, e)
    k = min(m, n)
    big = k > 512
    # the oracle on the scaled input: dgeqrf / dgerqf cope
    Qo, Ro = ref.qr(A)
    assert _finite(Qo, Ro) and _rel(Qo @ np.ldexp(Ro, -e), A0) <= TOL
    R2o, Q2o = ref.rq(A)
    assert _finite(Q2o, R2o) and _rel(np.ldexp(R2o, -e) @ Q2o, A0) <= TOL
    if m >= n or not big:   # (above 512 only the Gram-based direction: tall QR, wide RQ, as test_qr_rq_above_512)
        Q, R = handle.qr(handle.array(A))
        Qh, Rh = Q.numpy(), R.numpy()
        assert _finite(Qh, Rh)
        R1 = np.ldexp(Rh, -e)
        print(f"qr {m}x{n} e={e}: residual {_rel(Qh @ R1, A0):.2e} orthogonality {np.abs(Qh.T @ Qh - np.eye(k)).max():.2e}")
        assert _rel(Qh @ R1, A0) <= TOL
        assert _orth_ok(Qh.T @ Qh, k, big)
        assert np.allclose(np.tril(R1, -1), 0.0)   # upper triangular / trapezoidal
    if m <= n or not big:
        R2, Q2 = handle.rq(handle.array(A))
        R2h, Q2h = R2.numpy(), Q2.numpy()
        assert _finite(Q2h, R2h)
        R21 = np.ldexp(R2h, -e)
        print(f"rq {m}x{n} e={e}: residual {_rel(R21 @ Q2h, A0):.2e} orthogonality {np.abs(Q2h @ Q2h.T - np.eye(k)).max():.2e}")
        assert _rel(R21 @ Q2h, A0) <= TOL
        assert _orth_ok(Q2h @ Q2h.T, k, big)
        # this RQ is the transposed QR of A^T: its triangular factor is lower triangular / trapezoidal
        assert np.allclose(np.triu(R21, 1), 0.0)


# ------------------------------------------------------------------------------------------------ QC / CQ
def _rank17(m, n, sign):
    """Exactly rank 17: 17 random columns (tall) / rows (wide) in random positions, zeros elsewhere, as
    test_qc_cq_rank_deficient_above_512 (a product of random factors leaves the oracle's own rank a rounding
    accident of the 16 eps rule)."""
    rng = np.random.default_rng(m + n + 17)
    A = np.zeros((m, n))
    if m >= n:
        A[:, rng.permutation(n)[:17]] = rng.standard_normal((m, 17))
    else:
        A[rng.permutation(m)[:17], :] = rng.standard_normal((17, n))
    return sign * A


QC_CASES = [("random", m, n, e) for (m, n, _e) in QR_CASES for e in [_e]] + \
           [(kind, m, n, e) for kind in ("rank17+", "rank17-") for (m, n) in [(300, 40), (40, 300)] for e in SCALES]


@pytest.mark.parametrize("kind,m,n,e", QC_CASES)
def test_qc_cq(handle, ref, kind, m, n, e):
    if kind == "random":
        A0 = _cached(("qc", m, n), lambda: np.random.default_rng(m * 31 + n).standard_normal((m, n)))
    else:
        A0 = _cached((kind, m, n), lambda: _rank17(m, n, 1.0 if kind.endswith("+") else -1.0))
    A = np.ldexp(A0, e)
    big = min(m, n) > 512
    res_bar = TOL if kind == "random" else 1e-11   # (test_qc_random / the rank-deficient tests)
    if m >= n or not big:   # (above 512 only the Gram-based direction)
        r0 = _cached(("qc-rank", kind, m, n), lambda: ref.qc(A0)[2])
        Qo, Co, ro = ref.qc(A)
        assert ro == r0 and _rel(Qo @ np.ldexp(Co, -e), A0) <= res_bar   # the reference copes
        Q, Cm, r = handle.qc(handle.array(A))
        Qh, Ch = Q.numpy(), Cm.numpy()
        assert _finite(Qh, Ch)
        print(f"qc {kind} {m}x{n} e={e}: rank {r} (oracle {r0}) residual {_rel(Qh @ np.ldexp(Ch, -e), A0):.2e}")
        assert r == r0
        if kind == "random":
            assert r == min(m, n)
        assert _rel(Qh @ np.ldexp(Ch, -e), A0) <= res_bar
        assert _orth_ok(Qh.T @ Qh, r, big) if not big else np.abs(Qh.T @ Qh - np.eye(r)).max() <= 1e-12
    if m <= n or not big:
        r0 = _cached(("cq-rank", kind, m, n), lambda: ref.cq(A0)[2])
        Co, Qo, ro = ref.cq(A)
        assert ro == r0 and _rel(np.ldexp(Co, -e) @ Qo, A0) <= res_bar
        Cm, Q, r = handle.cq(handle.array(A))
        Ch, Qh = Cm.numpy(), Q.numpy()
        assert _finite(Qh, Ch)
        print(f"cq {kind} {m}x{n} e={e}: rank {r} (oracle {r0}) residual {_rel(np.ldexp(Ch, -e) @ Qh, A0):.2e}")
        assert r == r0
        if kind == "random":
            assert r == min(m, n)
        assert _rel(np.ldexp(Ch, -e) @ Qh, A0) <= res_bar
        assert _orth_ok(Qh @ Qh.T, r, big) if not big else np.abs(Qh @ Qh.T - np.eye(r)).max() <= 1e-12


def test_rank17_exercises_both_branches_of_the_rank_rule(ref):
    """The reference cuts only when its R_00 is positive: over the two signs both ranks (17 and 40) occur."""
    for m, n in [(300, 40), (40, 300)]:
        assert {ref.qc(_rank17(m, n, s))[2] for s in (1.0, -1.0)} == {17, 40}
        assert {ref.cq(_rank17(m, n, s))[2] for s in (1.0, -1.0)} == {17, 40}


# ------------------------------------------------------------------------------------------------ Jacobi rows
@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("p,q", [(17, 40), (129, 129)])
def test_svd_rows_vt(handle, ref, p, q, kernel, e):
    """The truncating round's Jacobi SVD (one workgroup / block kernel), graded spectrum as in a TT edge, at
    the bars of test_svd_rows_vt_kernels."""

    def make():
        rng = np.random.default_rng(p * 7 + q)
        U0, _ = np.linalg.qr(rng.standard_normal((p, p)))
        V0, _ = np.linalg.qr(rng.standard_normal((q, p)))
        s0 = np.logspace(0, -9, p)
        return (U0 * s0) @ V0.T, s0

    A0, s0 = _cached(("rows", p, q), make)
    A = np.ldexp(A0, e)
    So = ref.svd(A)[1]   # the reference copes
    assert np.abs(np.ldexp(So, -e) - s0).max() <= 1e-14 * s0[0] * np.sqrt(p)
    S, Vt, sweeps = handle.svd_rows_vt(handle.array(A), kernel)
    S, Vt = S.numpy(), Vt.numpy()
    assert _finite(S, Vt)
    S1 = np.ldexp(S, -e)
    print(f"svd_rows_vt {p}x{q} kernel {kernel} e={e}: sweeps {sweeps} S {np.abs(S1 - s0).max():.2e}")
    assert 0 < sweeps <= 40
    assert np.all(np.diff(S) <= 0)
    assert np.abs(S1 - s0).max() <= 1e-14 * s0[0] * np.sqrt(p)
    assert np.linalg.norm(Vt @ Vt.T - np.eye(p)) <= 1e-13 * p
    assert _rel((A0 @ Vt.T) @ Vt, A0) <= 1e-14 * np.sqrt(p)


# ------------------------------------------------------------------------------------------------ eigensolver
@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("n", [24, 128, 200])
def test_sym_eig_top(handle, n, e):
    """The kk = n / 2 largest eigenpairs of a symmetric matrix against LAPACK (scipy.linalg.eigh of the unscaled
    matrix, and of the scaled one: it copes), at the bars of test_syev_gpu.py."""

    def make():
        rng = np.random.default_rng(n)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * np.linspace(1.0, 5.0, n)) @ Q.T
        A = 0.5 * (A + A.T)
        return A, eigh(A, eigvals_only=True)[::-1]

    A0, w0 = _cached(("eig", n), make)
    kk = n // 2
    nrm = w0[0]   # ||A0||_2 (positive definite)
    A = np.ldexp(A0, e)
    wo = eigh(A, eigvals_only=True)[::-1]
    assert np.abs(np.ldexp(wo, -e) - w0).max() <= 1e-13 * nrm
    lam, Ut, st = handle.sym_eig_top(handle.array(A), kk)
    lam, U = lam.numpy(), Ut.numpy().T
    assert st == 0
    assert _finite(lam, U)
    lam1 = np.ldexp(lam, -e)
    print(f"sym_eig_top n={n} e={e}: eigenvalues {np.abs(lam1 - w0[:kk]).max() / nrm:.2e}")
    assert np.abs(lam1 - w0[:kk]).max() <= 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(kk)).max() <= 1e-12
    assert np.linalg.norm(A0 @ U - U * lam1, axis=0).max() <= 1e-12 * nrm


# ------------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("m,n", [(30, 30), (60, 30)])
def test_solve(handle, m, n, e):
    """A X = B with A and B = A X0 both at 2^e: X = X0 at the 1e-10 of test_solve_general_and_least_squares,
    through xrs_solve and xrs_solve_least_squares."""
    def make():
        rng = np.random.default_rng(m * 13 + n)
        A = rng.standard_normal((m, n))
        X = rng.standard_normal((n, 2))
        return A, X, A @ X

    A0, X0, B0 = _cached(("solve", m, n), make)
    A, B = np.ldexp(A0, e), np.ldexp(B0, e)
    # the reference's dgelsd on the scaled system
    Xo = np.linalg.lstsq(A, B, rcond=None)[0]
    assert _rel(Xo, X0) <= 1e-10
    for ls in (False, True):
        X = handle.solve(handle.array(A), handle.array(B), least_squares=ls).numpy()
        assert _finite(X)
        print(f"solve {m}x{n} e={e} least_squares={ls}: {_rel(X, X0):.2e}")
        assert _rel(X, X0) <= 1e-10


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("e", SCALES + [SUB])
@pytest.mark.parametrize("n", [1, 255, 1025, 5000])
def test_nrm2_asum(handle, n, e):
    """xrs_nrm2 / xrs_asum against dnrm2 / dasum (the reference's two_norm / one_norm), rtol 1e-14 as
    test_kernels_gpu.py."""
    x0 = _cached(("vec", n), lambda: np.random.default_rng(n).standard_normal(n))
    x, x1 = _unscaled(x0, e)
    want2, want1 = float(dnrm2(x1)), float(dasum(x1))
    o2, o1 = float(dnrm2(x)), float(dasum(x))   # the reference on the scaled data
    dev2, dev1 = abs(np.ldexp(o2, -e) - want2) / want2, abs(np.ldexp(o1, -e) - want1) / want1
    bar2 = bar1 = 1e-14
    if e == SUB:
        bar2, bar1 = max(bar2, 8 * dev2), max(bar1, 8 * dev1)
    else:
        assert dev2 <= bar2 and dev1 <= bar1
    dx = handle.array(x)
    g2, g1 = handle.nrm2(dx), handle.asum(dx)
    print(f"nrm2/asum n={n} e={e}: {abs(np.ldexp(g2, -e) - want2) / want2:.2e} {abs(np.ldexp(g1, -e) - want1) / want1:.2e}"
          f" (oracle {dev2:.2e} {dev1:.2e})")
    assert np.isfinite(g2) and np.isfinite(g1)
    assert abs(np.ldexp(g2, -e) - want2) <= bar2 * want2
    assert abs(np.ldexp(g1, -e) - want1) <= bar1 * want1


@pytest.mark.parametrize("e", [0, 600, -600])
def test_nrm2_keeps_a_nan(handle, e):
    """A NaN entry is the norm, as in dnrm2, whichever of the scaled accumulators the other entries reach."""
    x = np.ldexp(np.random.default_rng(7).standard_normal(300), e)
    x[123] = np.nan
    assert np.isnan(dnrm2(x))
    assert np.isnan(handle.nrm2(handle.array(x)))


# ------------------------------------------------------------------------------------------------ TT
TT_DIMS, TT_RANKS = [6] * 5, [8] * 4
# variant A: core 2 at 2^e; variant B: every core at 2^+-160 (2^+-800 in all: the scale accumulates along a sweep)
TT_VARIANTS = {"A+600": [0, 0, 600, 0, 0], "A-600": [0, 0, -600, 0, 0], "A+830": [0, 0, 830, 0, 0],
               "A-830": [0, 0, -830, 0, 0], "B+160": [160] * 5, "B-160": [-160] * 5}
TT_OPS = {"move_core(0)": [6, 8, 8, 6], "move_core(4)": [6, 8, 8, 6], "round(4)": [4, 4, 4, 4], "round(8,eps=0.3)": [4, 7, 6, 3]}


def _tt_apply(x, op):
    """The op on an oracle TT or a TTDevice; returns the core position."""
    if op == "move_core(0)":
        x.move_core(0)
        return 0
    if op == "move_core(4)":
        x.move_core(4)
        return 4
    if op == "round(4)":
        x.round(4)
    else:
        x.round([8] * 4, eps=0.3)
    return 0


def _tt_diff_norm(ref, a_cores, b_cores):
    """(||A - B||, ||B||) without cancellation, as tests/test_tt_gpu.py: the difference TT orthogonalised by
    the oracle and its norm read off the core."""
    A = ref.TT([c.copy() for c in a_cores])
    B = ref.TT([c.copy() for c in b_cores])
    nb = [c.copy() for c in B.cores]
    nb[0] = -nb[0]
    D = ref.tt_add(A, ref.TT(nb))
    D.move_core(0)
    B.move_core(0)
    return D.frob_norm(), B.frob_norm()


@pytest.mark.parametrize("op", list(TT_OPS))
@pytest.mark.parametrize("variant", list(TT_VARIANTS))
def test_tt(handle, ref, variant, op):
    x0 = _cached("tt", lambda: ref.TT.random_raw(TT_DIMS, TT_RANKS, ref.Rng(41)))
    exps = TT_VARIANTS[variant]
    total = sum(exps)

    def oracle():
        y = x0.copy()
        _tt_apply(y, op)
        return y, y.frob_norm()

    y0, norm0 = _cached(("tt", op), oracle)
    assert y0.ranks == TT_OPS[op]
    scaled = [np.ldexp(c, ex) for c, ex in zip(x0.cores, exps)]
    # the oracle on the scaled TT: same ranks, same tensor, the norm scaled exactly
    ys = ref.TT([c.copy() for c in scaled])
    pos = _tt_apply(ys, op)
    assert ys.ranks == y0.ranks
    yc = [c.copy() for c in ys.cores]
    yc[pos] = np.ldexp(yc[pos], -total)
    diff, nrm = _tt_diff_norm(ref, yc, y0.cores)
    assert _finite(*ys.cores) and diff <= 1e-12 * nrm
    assert abs(np.ldexp(ys.frob_norm(), -total) - norm0) <= 1e-12 * norm0

    g = capi.TTDevice.from_cores(handle, scaled)
    assert _tt_apply(g, op) == pos
    path = handle.last_round_path() if op.startswith("round") else None
    gc = g.cores()
    print(f"tt {variant} {op}: ranks {g.ranks} (oracle {y0.ranks}) path {path}")
    assert g.ranks == y0.ranks
    assert _finite(*gc)
    fn = g.frob_norm()
    gc[pos] = np.ldexp(gc[pos], -total)
    for k, c in enumerate(gc):   # canonical form: every core but the one at `pos` orthonormal
        if k < pos:
            M = c.reshape(-1, c.shape[2])
            assert np.abs(M.T @ M - np.eye(M.shape[1])).max() <= 1e-12
        elif k > pos:
            M = c.reshape(c.shape[0], -1)
            assert np.abs(M @ M.T - np.eye(M.shape[0])).max() <= 1e-12
    if op.startswith("move_core"):
        diff, nrm = _tt_diff_norm(ref, gc, y0.cores)
        print(f"tt {variant} {op}: difference {diff / nrm:.2e}")
        assert diff <= 1e-12 * nrm
    else:   # truncating: the truncation errors agree (test_round_truncating), and so do the results themselves
        e_ref, nrm = _cached(("tt-err", op), lambda: _tt_diff_norm(ref, y0.cores, x0.cores))
        e_gpu, _ = _tt_diff_norm(ref, gc, x0.cores)
        diff, nrm_y = _tt_diff_norm(ref, gc, y0.cores)
        print(f"tt {variant} {op}: truncation error {e_gpu / nrm:.6e} (oracle {e_ref / nrm:.6e}), difference {diff / nrm_y:.2e}")
        assert abs(e_gpu - e_ref) <= 1e-6 * nrm
        assert diff <= 1e-10 * nrm_y
    print(f"tt {variant} {op}: frob_norm {abs(np.ldexp(fn, -total) - norm0) / norm0:.2e}")
    assert np.isfinite(fn) and abs(np.ldexp(fn, -total) - norm0) <= 1e-12 * norm0


# a TT within its maximal ranks and a round with nothing to cut: the certified chain pass (Gram chains over all
# cores, batched Cholesky, no SVD). Its Grams are inf (A+600, B+160), zero (A-600, B-160) or subnormal with a
# third of their digits (A-520: 2^-1040); the certificates or the orthogonality check must turn those away.
CHAIN_VARIANTS = dict(TT_VARIANTS, **{"A-520": [0, 0, -520, 0, 0], "none": [0] * 5})


@pytest.mark.parametrize("variant", list(CHAIN_VARIANTS))
def test_tt_round_nothing_to_cut(handle, ref, variant):
    ranks = [6, 8, 8, 6]
    x0 = _cached("tt-chain", lambda: ref.TT.random_raw(TT_DIMS, ranks, ref.Rng(43)))
    exps = CHAIN_VARIANTS[variant]
    total = sum(exps)

    def oracle():
        y = x0.copy()
        y.round(8)
        return y, y.frob_norm()

    y0, norm0 = _cached("tt-chain-oracle", oracle)
    assert y0.ranks == ranks
    scaled = [np.ldexp(c, ex) for c, ex in zip(x0.cores, exps)]
    ys = ref.TT([c.copy() for c in scaled])   # the reference copes
    ys.round(8)
    assert ys.ranks == ranks and abs(np.ldexp(ys.frob_norm(), -total) - norm0) <= 1e-12 * norm0
    g = capi.TTDevice.from_cores(handle, scaled)
    g.round(8)
    path = handle.last_round_path()
    gc = g.cores()
    print(f"tt chain {variant}: ranks {g.ranks} path {path}")
    assert g.ranks == ranks
    assert _finite(*gc)
    if variant == "none":
        assert path == "chain"
    fn = g.frob_norm()
    gc[0] = np.ldexp(gc[0], -total)
    for c in gc[1:]:   # right-canonical, at the bar of test_round_non_truncating
        M = c.reshape(c.shape[0], -1)
        assert np.linalg.norm(M @ M.T - np.eye(M.shape[0])) <= 1e-12 * M.shape[0]
    diff, nrm = _tt_diff_norm(ref, gc, x0.cores)
    print(f"tt chain {variant}: difference {diff / nrm:.2e} frob_norm {abs(np.ldexp(fn, -total) - norm0) / norm0:.2e}")
    assert diff <= 1e-10 * nrm
    assert np.isfinite(fn) and abs(np.ldexp(fn, -total) - norm0) <= 1e-12 * norm0
