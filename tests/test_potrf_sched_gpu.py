"""The two bodies of the register-resident Cholesky (n <= 256, csrc/smallla.hip): the default critical-tiles-first
body (potrf_cf_body) against the plain right-looking one (potrf_rr_body, XRS_POTRF_BODY=plain, read at every call).
The schedules differ, the arithmetic of every tile does not: L, the inverse built from the diagonal-block inverses
and the statuses must be equal byte for byte, at every order where tile ownership changes, in place (xrs_potrf_solve),
out of place and as status-only certificate jobs (xrs_chol_batch), and in one batched launch of mixed orders. On
failing inputs the statuses must be equal and be what the contract states: 1 + the first failing column (a pivot
outside (0, 1e300)), 1 for a zero matrix, nonzero for a non-finite entry. Inputs are fixed by their seeds."""
import functools

import numpy as np
import pytest

import chol_ref as cr

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 129, 240, 255, 256)
SHIFTS = (0.0, 1.0e-11)
BATCH = (256, 20, 256, 1, 17, 100, 255)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def matrices(n):
    """(name, A, status of the long-double reference per shift) of the two SPD inputs of an order."""
    out = []
    for name, kappa, seed in (("k1e2", 1.0e2, 1000 + n), ("k1e8", 1.0e8, 2000 + n)):
        A = cr.spd(n, cr.graded(n, kappa), seed)
        out.append((name, A, tuple(cr.chol_ld(A, s)[1] for s in SHIFTS + (-cr.TAU,))))
    return tuple(out)


def batch(handle, jobs, mode):
    """jobs: (A, shift, want_L, want_Z); one xrs_chol_batch call. Returns [(status, L, Z)] (None where not asked)."""
    dA = [handle.array(A) for A, _, _, _ in jobs]
    dL = [handle.array(np.full(A.shape, -7.0)) if wl else None for A, _, wl, _ in jobs]
    dZ = [handle.array(np.full(A.shape, -7.0)) if wz else None for A, _, _, wz in jobs]
    status, _ = handle.chol_batch([d.ptr for d in dA], [d.ptr if d else 0 for d in dL], [d.ptr if d else 0 for d in dZ],
                                  [A.shape[0] for A, _, _, _ in jobs], [s for _, s, _, _ in jobs], mode)
    out = [(status[i], dL[i].numpy() if dL[i] else None, dZ[i].numpy() if dZ[i] else None) for i in range(len(jobs))]
    for d in dA + dL + dZ:
        if d:
            d.free()
    return out


def in_place(handle, A, shift):
    """xrs_potrf_solve: potrf in place on a copy of A, then X = L^{-1} I through the diagonal-block inverses (trsm).
    Returns (status, L, X)."""
    n = A.shape[0]
    dA, dL, dY, dX = handle.array(A), handle.array(np.full((n, n), -7.0)), handle.array(np.eye(n)), handle.array(np.full((n, n), -7.0))
    st, _ = handle.potrf_solve(dL.ptr, dA.ptr, n, shift, True, dY.ptr, n, dX.ptr, n, n)
    out = (st, dL.numpy(), dX.numpy())
    for d in (dA, dL, dY, dX):
        d.free()
    return out


def both_bodies(monkeypatch, fn):
    """fn() under the default body and under the plain one."""
    monkeypatch.delenv("XRS_POTRF_BODY", raising=False)
    new = fn()
    monkeypatch.setenv("XRS_POTRF_BODY", "plain")
    plain = fn()
    monkeypatch.delenv("XRS_POTRF_BODY")
    return new, plain


def assert_same_results(tag, new, plain, with_bytes=True):
    assert len(new) == len(plain)
    for i, (a, b) in enumerate(zip(new, plain)):
        assert a[0] == b[0], (tag, i, "status", a[0], b[0])
        if not with_bytes:
            continue
        for which in (1, 2):
            assert (a[which] is None) == (b[which] is None)
            if a[which] is not None:
                assert same(a[which], b[which]), (tag, i, "LZ"[which - 1], "bodies differ")


@pytest.mark.parametrize("n", ORDERS)
def test_bodies_agree_byte_for_byte(handle, monkeypatch, n):
    """kappa = 100 and a graded kappa = 1e8, shifts 0 and 1e-11: out of place with and without the inverse, status-only
    (with the certificate's shift as well), the bare batch tables, and in place."""
    jobs, expect = [], []
    for name, A, ref_status in matrices(n):
        for si, s in enumerate(SHIFTS):
            jobs += [(A, s, True, True), (A, s, True, False), (A, s, False, False)]
            expect += [ref_status[si]] * 3
        jobs.append((A, -cr.TAU, False, False))
        expect.append(ref_status[2])
    assert expect == [0] * len(jobs)   # (the reference decides every job; none is a failure case)
    for mode in (0, 2):
        new, plain = both_bodies(monkeypatch, lambda: batch(handle, jobs, mode))
        assert [r[0] for r in new] == expect, (n, mode, [r[0] for r in new])
        assert_same_results(("batch", n, mode), new, plain)
    for name, A, _ in matrices(n):
        for s in SHIFTS:
            new, plain = both_bodies(monkeypatch, lambda: [in_place(handle, A, s)])
            assert new[0][0] == 0
            assert_same_results(("in place", n, name, s), new, plain)
            assert np.array_equal(new[0][1][np.triu_indices(n, 1)], np.zeros(n * (n - 1) // 2))


@pytest.mark.parametrize("n", (300, 520))
def test_bodies_agree_in_the_block_paths(handle, monkeypatch, n):
    """The 2 x 2 class and chol_full factor their diagonal blocks with the same kernels."""
    A = cr.well(n)[0]
    jobs = [(A, 0.0, True, True), (A, -cr.TAU, False, False)]
    new, plain = both_bodies(monkeypatch, lambda: batch(handle, jobs, 0))
    assert [r[0] for r in new] == [0, 0]
    assert_same_results(("block path", n), new, plain)


def failure_columns(n):
    """First failing columns (1-based): 1, both sides of the first tile edge, the second edge, the last tile, n."""
    return sorted({c for c in (1, 16, 17, 32, 241, n) if c <= n})


def run_failure(handle, monkeypatch, tag, A, expect):
    """The three forms under both bodies: equal statuses; expect: the status, or None for "nonzero"."""
    jobs = [(A, 0.0, True, True), (A, 0.0, False, False)]
    for mode in (0, 2):
        new, plain = both_bodies(monkeypatch, lambda: batch(handle, jobs, mode))
        assert_same_results((tag, mode), new, plain, with_bytes=False)
        for st, _, _ in new:
            assert st == expect if expect is not None else st != 0, (tag, mode, st, expect)
    new, plain = both_bodies(monkeypatch, lambda: [in_place(handle, A, 0.0)])
    assert_same_results((tag, "in place"), new, plain, with_bytes=False)
    assert new[0][0] == expect if expect is not None else new[0][0] != 0, (tag, "in place", new[0][0], expect)


@pytest.mark.parametrize("n", (17, 100, 256))
def test_failure_statuses_agree(handle, monkeypatch, n):
    for c in failure_columns(n):
        A = cr.indefinite_at(n, c - 1, 4000 + n)
        assert cr.chol_ld(A)[1] == c
        run_failure(handle, monkeypatch, ("indefinite", n, c), A, c)
    run_failure(handle, monkeypatch, ("zero", n), np.zeros((n, n)), 1)
    k = n // 2
    for bad in (np.nan, np.inf, -np.inf, 2.0e300):
        A = cr.well(n)[0].copy()
        A[k, k] = bad
        run_failure(handle, monkeypatch, ("non-finite", n, bad), A, k + 1 if np.isfinite(bad) else None)
    A = cr.well(n)[0].copy()
    A[n - 1, 0] = np.nan   # an off-diagonal NaN reaches the pivots of its row
    run_failure(handle, monkeypatch, ("nan off the diagonal", n), A, None)


def test_one_batched_launch_of_mixed_orders(handle, monkeypatch):
    """n = (256, 20, 256, 1, 17, 100, 255) in one launch: each job's bytes are those of the job alone, under both
    bodies, and the two bodies' are equal. A failing job among them does not disturb its neighbours."""
    jobs = [(cr.well(n)[0] if i != 2 else cr.spd(n, cr.graded(n, 1.0e8), 2000 + n), 0.0, True, True) for i, n in enumerate(BATCH)]
    for mode in (0, 2):
        new, plain = both_bodies(monkeypatch, lambda: batch(handle, jobs, mode))
        assert [r[0] for r in new] == [0] * len(jobs)
        assert_same_results(("mixed", mode), new, plain)
        alone_new, alone_plain = both_bodies(monkeypatch, lambda: [batch(handle, [job], mode)[0] for job in jobs])
        assert_same_results(("mixed against alone", mode), new, alone_new)
        assert_same_results(("mixed against alone, plain", mode), plain, alone_plain)
    broken = list(jobs)
    broken[4] = (cr.indefinite_at(17, 16, 4017), 0.0, True, True)
    new, plain = both_bodies(monkeypatch, lambda: batch(handle, broken, 2))
    assert [r[0] for r in new] == [0, 0, 0, 0, 17, 0, 0] == [r[0] for r in plain]
    good = [i for i in range(len(jobs)) if i != 4]
    assert_same_results("mixed with a failing job", [new[i] for i in good], [plain[i] for i in good])
    alone = batch(handle, jobs, 2)
    assert_same_results("neighbours of a failing job", [new[i] for i in good], [alone[i] for i in good])
