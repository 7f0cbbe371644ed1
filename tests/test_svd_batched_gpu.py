"""xrs_svd_batched (svd_batched.hip: one workgroup per matrix, one-sided Jacobi in LDS with the rotations
accumulated, one launch and one synchronisation per batch) and calculate_svd_batched, against LAPACK per member.

The bars are xrs_svd's own (test_svd_bidiag_gpu.py, test_range_scaling_gpu.py): |S - S_ref| <= 1e-12 max(S_ref[0], 1),
||U S Vt - A|| <= 1e-14 ||A||, max |U^T U - I| and max |Vt Vt^T - I| <= 1e-14, S non-increasing. status[b] >= 0
means the batched kernel produced member b; -1 that the single-matrix route recomputed it.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (1, 7), (7, 1), (5, 3), (3, 5), (16, 16), (17, 33), (33, 17), (64, 64), (32, 256), (40, 100), (100, 40)]
BATCHES = [1, 3, 37]


def _gauss(shape, batch, seed=0):
    """The seeded Gaussian batches of this file (every member has cond <= 1e6: checked on the CPU, the largest
    is 2.3e4, a 64 x 64 member)."""
    m, n = shape
    return np.random.default_rng([seed, m, n, batch]).standard_normal((batch, m, n))


def _run(handle, A, want_status=True):
    U, S, Vt, st = handle.svd_batched(handle.array(A), want_status)
    return U.numpy(), S.numpy(), Vt.numpy(), st


def _check_member(A, U, S, Vt):
    """xrs_svd's bars for one member, relative to the member's own ||A|| and S_ref[0] (entries scaled by
    1 / max |A| before norms are formed, as test_svd_bidiag_gpu.py does, so 1e+-150-sized members do not
    overflow the check itself)."""
    m, n = A.shape
    k = min(m, n)
    assert U.shape == (m, k) and S.shape == (k,) and Vt.shape == (k, n)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(Vt))
    assert np.all(np.diff(S) <= 0) and np.all(S >= 0)
    amax = np.abs(A).max()
    sc = 1.0 / amax if amax > 0 else 1.0
    Sr = np.linalg.svd(A * sc, compute_uv=False)
    assert np.abs(S * sc - Sr).max() <= 1e-12 * max(Sr[0], 1.0)
    assert np.linalg.norm((U * (S * sc)) @ Vt - A * sc) <= 1e-14 * np.linalg.norm(A * sc)
    assert np.abs(U.T @ U - np.eye(k)).max() <= 1e-14
    assert np.abs(Vt @ Vt.T - np.eye(k)).max() <= 1e-14


def _check_batch(A, U, S, Vt):
    for b in range(A.shape[0]):
        _check_member(A[b], U[b], S[b], Vt[b])


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_batches(handle, shape, batch):
    A = _gauss(shape, batch)
    U, S, Vt, st = _run(handle, A)
    assert st.shape == (batch,) and np.all(st >= 0), st   # the kernel, not the fallback
    _check_batch(A, U, S, Vt)


def test_more_workgroups_than_cus(handle):
    A = _gauss((16, 16), 300)
    U, S, Vt, st = _run(handle, A)
    assert np.all(st >= 0), st
    _check_batch(A, U, S, Vt)


def test_members_independent_and_deterministic(handle):
    A = _gauss((17, 33), 37)
    A[11] = A[5]   # two identical members
    U, S, Vt, st = _run(handle, A)
    assert np.all(st >= 0)
    for b in range(37):
        U1, S1, Vt1, st1 = _run(handle, A[b:b + 1])
        assert st1[0] == st[b]
        assert np.array_equal(U1[0], U[b]) and np.array_equal(S1[0], S[b]) and np.array_equal(Vt1[0], Vt[b])
    assert np.array_equal(U[11], U[5]) and np.array_equal(S[11], S[5]) and np.array_equal(Vt[11], Vt[5])


def test_per_matrix_scaling(handle):
    A = _gauss((16, 16), 5, seed=1)
    for b, f in enumerate([1e-150, 1.0, 1e150, 2.0 ** -400, 2.0 ** 400]):
        A[b] *= f
    U, S, Vt, st = _run(handle, A)
    assert np.all(st >= 0), st
    _check_batch(A, U, S, Vt)


def test_certificate_and_fallback_inside_a_batch(handle):
    rng = np.random.default_rng(7)
    n = 16
    A = _gauss((n, n), 5, seed=2)
    # exactly rank 2 (small integers: the products and sums are exact), zero, graded 1 .. 1e-13
    A[2] = rng.integers(-4, 5, (n, 2)).astype(float) @ rng.integers(-4, 5, (2, n)).astype(float)
    assert np.linalg.matrix_rank(A[2]) == 2
    A[3] = 0.0
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A[4] = (Q1 * np.logspace(0, -13, n)) @ Q2.T
    U, S, Vt, st = _run(handle, A)
    _check_batch(A, U, S, Vt)   # (includes full orthonormal U and Vt of the rank-2 and the zero member)
    assert st[0] >= 0 and st[1] >= 0, st
    assert st[2] == -1 and st[3] == -1, st
    assert not S[3].any() and np.all(S[2][2:] <= 1e-12 * S[2][0])


def test_outside_the_envelope(handle):
    from xerus_amd import capi

    assert not capi.svd_batched_fits(130, 130) and not capi.svd_batched_fits(128, 128)
    assert capi.svd_batched_fits(64, 64) and capi.svd_batched_fits(32, 448) and capi.svd_batched_fits(448, 32)
    A = _gauss((130, 130), 2)
    U, S, Vt, st = _run(handle, A)
    assert list(st) == [-1, -1]
    _check_batch(A, U, S, Vt)


def test_batch_zero_and_null_status(handle):
    from xerus_amd.capi import _DP

    # batch 0: status 0, nothing written (also not to the status array)
    m, n = 5, 3
    sentinel = np.full(m * n, 7.25)
    U, S, Vt, A = (handle.array(sentinel[:c]) for c in (m * n, n, n * n, m * n))
    st = np.full(4, 99, dtype=np.intc)
    rc = handle.lib.xrs_svd_batched(handle.h, _DP(U.ptr), _DP(S.ptr), _DP(Vt.ptr), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                    _DP(A.ptr), 0, m, n)
    assert rc == 0
    assert np.all(st == 99)
    for d in (U, S, Vt):
        assert np.all(d.numpy() == 7.25)
    Ue, Se, Vte, ste = _run(handle, np.zeros((0, m, n)))
    assert Ue.shape == (0, m, n) and Se.shape == (0, n) and Vte.shape == (0, n, n) and ste.shape == (0,)
    # status = NULL
    B = _gauss((5, 3), 3)
    Ub, Sb, Vtb, none = _run(handle, B, want_status=False)
    assert none is None
    _check_batch(B, Ub, Sb, Vtb)


def _spectrum_tensor(rng, dims, split, s):
    """A tensor whose unfolding at `split` has the singular values s."""
    m, n = int(np.prod(dims[:split])), int(np.prod(dims[split:]))
    k = min(m, n)
    Q1, _ = np.linalg.qr(rng.standard_normal((m, k)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return ((Q1 * s[:k]) @ Q2.T).reshape(dims)


@pytest.mark.parametrize("split", [1, 2])
def test_calculate_svd_batched(xe, split):
    rng = np.random.default_rng(21)
    dims = [(4, 5, 6), (6, 5, 4), (4, 5, 6), (6, 5, 4), (6, 5, 4), (4, 5, 6)]   # mixed shapes, interleaved
    gauss = [rng.standard_normal(d) for d in dims]
    # known spectrum 1, 1/2, 1/4, 1e-4, 1e-5, ...: eps = 1e-3 cuts at rank 3
    spec = np.concatenate([[1.0, 0.5, 0.25], 10.0 ** -np.arange(4.0, 40.0)])
    graded = [_spectrum_tensor(rng, d, split, spec) for d in dims]

    def tensors(arrays):
        ts = [xe.Tensor.from_ndarray(a) for a in arrays]
        ts[1] = ts[1] * -2.0   # one input carries a negative factor
        assert ts[1].factor == -2.0
        return ts

    for arrays, max_rank, eps, want_rank in ((gauss, 0, xe.EPSILON, None), (gauss, 3, xe.EPSILON, 3), (graded, 0, 1e-3, 3)):
        ts = tensors(arrays)
        before = [(t.factor, t.to_ndarray()) for t in ts]
        out = xe.calculate_svd_batched(ts, split, max_rank, eps)
        assert len(out) == len(ts)
        for t, (f0, a0) in zip(ts, before):   # the inputs are unchanged
            assert t.factor == f0 and np.array_equal(t.to_ndarray(), a0)
        for t, (f0, a0), (U, S, Vt) in zip(ts, before, out):
            U1, S1, Vt1 = xe.calculate_svd(t, split, max_rank, eps)
            assert U.dimensions == U1.dimensions and S.dimensions == S1.dimensions and Vt.dimensions == Vt1.dimensions
            r = S.dimensions[0]
            if want_rank is not None:
                assert r == want_rank
            s, s1 = np.diag(S.to_ndarray()), np.diag(S1.to_ndarray())
            assert np.abs(s - s1).max() <= 1e-12 * s1[0]
            m = int(np.prod(a0.shape[:split]))
            full = U.to_ndarray().reshape(m, r) @ S.to_ndarray() @ Vt.to_ndarray().reshape(r, -1)
            full1 = U1.to_ndarray().reshape(m, r) @ S1.to_ndarray() @ Vt1.to_ndarray().reshape(r, -1)
            assert np.linalg.norm(full - full1) <= 1e-13 * np.linalg.norm(full1)
            if max_rank == 0 and want_rank is None:   # untruncated: the factors reproduce the input itself
                assert np.linalg.norm(full - a0.reshape(m, -1)) <= 1e-13 * np.linalg.norm(a0)
