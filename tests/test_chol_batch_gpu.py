"""The batched Cholesky family called directly (xrs_chol_batch: chol_enqueue / chol_enqueue_factors + _inverses /
potrf_batched + trinv_batched; xrs_potrf_solve: potrf + trsm) against the long-double reference of tests/chol_ref.py:
accuracy of L and Z = L^{-1} at every order where a mechanism changes, the status contract (1 + first failing column,
per job), certificates on both sides of tau tr A, the documented contracts (zeros above the diagonal, A untouched,
guard zones, lower triangle read) and the slot mapping of the batched launches.

Bars: 8 x the worst value the CPU references reach over the cases of a group, rounded up to a power of two
(tools/chol_bars.py prints them): LAPACK's float64 factor and inverse for the well-conditioned cases, the float64 blocked
emulation (explicit block inverses: only conditionally stable, so LAPACK is the wrong yardstick) for the graded ones.
test_chol_ref_cpu.py checks that no well-conditioned bar exceeds 16 n u and that every status and certificate input
is decided by the reference with a margin rounding cannot cross."""
import functools

import numpy as np
import pytest

import chol_ref as cr

pytestmark = pytest.mark.gpu

# ---- bars ------------------------------------------------------------------------------------------------------
# group: (res_L, res_Z, white).  Reference values (worst over the group, LAPACK float64, kappa = 100), and in
# brackets the worst values the kernels reached on an MI355X when the tests were written:
#   n1_2      res_L 8.29e-17  res_Z 2.80e-17  white 6.57e-16   (MI355X: 1.62e-16 / 1.11e-16 / 1.39e-16)
#   n15_17    res_L 9.26e-17  res_Z 2.89e-17  white 1.14e-15   (MI355X: 1.74e-16 / 3.48e-17 / 1.09e-15)
#   n31_49    res_L 1.00e-16  res_Z 3.08e-17  white 1.84e-15   (MI355X: 1.84e-16 / 2.79e-17 / 2.40e-15)
#   n100_129  res_L 1.44e-16  res_Z 2.57e-17  white 1.73e-15   (MI355X: 2.57e-16 / 1.74e-17 / 5.87e-15)
#   n240_256  res_L 1.84e-16  res_Z 2.47e-17  white 2.61e-15   (MI355X: 3.61e-16 / 1.21e-17 / 5.78e-15)
#   b2x2      res_L 2.50e-16  res_Z 2.48e-17  white 3.71e-15   (MI355X: 3.55e-16 / 1.25e-17 / 5.54e-15)
#   full      res_L 3.04e-16  res_Z 2.29e-17  white 5.22e-15   (MI355X: 3.10e-16 / 1.09e-17 / 3.98e-15)
#   k32       res_L 2.50e-16  res_Z 2.48e-17  white 3.43e-15   (MI355X: 1.72e-16 / 1.09e-17 / 1.72e-15)
BARS_WELL = {
    "n1_2": (2.0 ** -50, 2.0 ** -51, 2.0 ** -47),
    "n15_17": (2.0 ** -50, 2.0 ** -51, 2.0 ** -46),
    "n31_49": (2.0 ** -50, 2.0 ** -51, 2.0 ** -45),
    "n100_129": (2.0 ** -49, 2.0 ** -52, 2.0 ** -46),
    "n240_256": (2.0 ** -49, 2.0 ** -52, 2.0 ** -45),
    "b2x2": (2.0 ** -48, 2.0 ** -52, 2.0 ** -44),
    "full": (2.0 ** -48, 2.0 ** -52, 2.0 ** -44),
    "k32": (2.0 ** -48, 2.0 ** -52, 2.0 ** -45),
}
# graded spectra (kappa 1e4, 1e8 and lambda_min = 4 tau tr A), float64 blocked emulation with the path's block size:
#   rr        res_L 1.41e-16  res_Z 6.97e-17  white 9.45e-08   (MI355X: 2.92e-16 / 6.08e-17 / 6.48e-08)
#   b2x2      res_L 1.06e-15  res_Z 8.22e-17  white 1.20e-08   (MI355X: 6.26e-16 / 5.74e-17 / 3.34e-09)
#   full      res_L 8.70e-16  res_Z 7.14e-17  white 2.03e-09   (MI355X: 5.45e-16 / 4.59e-17 / 1.52e-09)
#   k32       res_L 1.69e-16  res_Z 6.85e-17  white 4.05e-09   (MI355X: 1.68e-16 / 4.86e-17 / 3.15e-09)
BARS_GRADED = {
    "rr": (2.0 ** -49, 2.0 ** -50, 2.0 ** -20),
    "b2x2": (2.0 ** -46, 2.0 ** -50, 2.0 ** -23),
    "full": (2.0 ** -47, 2.0 ** -50, 2.0 ** -25),
    "k32": (2.0 ** -49, 2.0 ** -50, 2.0 ** -24),
}
# ||X - L^{-1} Y||_F / ||L^{-1} Y||_F, LAPACK solve with LAPACK's factor of the same matrix:
#   n1_17     2.01e-16   (MI355X: 2.07e-16)
#   n100_256  4.18e-16   (MI355X: 2.63e-16)
#   n257_512  5.43e-16   (MI355X: 2.35e-16)
BARS_TRSM = {
    "n1_17": 2.0 ** -49,
    "n100_256": 2.0 ** -48,
    "n257_512": 2.0 ** -47,
}



def well_bars(n, k32=False):
    """The bars of a well-conditioned case of order n; none may exceed 16 n u."""
    return tuple(min(b, 16 * n * cr.U) for b in BARS_WELL[cr.well_group_of(n, k32)])


GUARD = 64
SENTINEL = -1.2345678901234567e77


def same(a, b):
    """Bit-identical (NaNs included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Guarded:
    """A device matrix between two guard zones of 64 sentinel doubles; the matrix itself starts as sentinels too."""

    def __init__(self, handle, shape):
        self.shape = tuple(shape)
        self.size = int(np.prod(self.shape))
        self.dev = handle.array(np.full(self.size + 2 * GUARD, SENTINEL))
        self.ptr = self.dev.ptr + 8 * GUARD

    def get(self):
        flat = self.dev.numpy()
        assert np.all(flat[:GUARD] == SENTINEL) and np.all(flat[GUARD + self.size:] == SENTINEL), "guard zone overwritten"
        return flat[GUARD:GUARD + self.size].reshape(self.shape)


def run_jobs(handle, jobs, mode):
    """jobs: (A, shift, want_L, want_Z). One xrs_chol_batch call. Returns ([(status, L, Z)], raw); L / Z are None
    where not asked for. Checks on every call: A bit-identical afterwards, guard zones intact, outputs that were not
    asked for do not exist (null pointers), and L, Z of a successful n <= 256 job exactly zero above the diagonal."""
    dA = [handle.array(A) for A, _, _, _ in jobs]
    ns = [A.shape[0] for A, _, _, _ in jobs]
    gL = [Guarded(handle, A.shape) if wl else None for A, _, wl, _ in jobs]
    gZ = [Guarded(handle, A.shape) if wz else None for A, _, _, wz in jobs]
    status, raw = handle.chol_batch([d.ptr for d in dA], [g.ptr if g else 0 for g in gL], [g.ptr if g else 0 for g in gZ],
                                    ns, [s for _, s, _, _ in jobs], mode)
    out = []
    for i, (A, _, _, _) in enumerate(jobs):
        assert same(dA[i].numpy(), A), "input matrix changed"
        L = gL[i].get() if gL[i] else None
        Z = gZ[i].get() if gZ[i] else None
        if status[i] == 0 and ns[i] <= 256:
            for M in (L, Z):
                if M is not None:
                    assert np.array_equal(M[np.triu_indices(ns[i], 1)], np.zeros(ns[i] * (ns[i] - 1) // 2)), "upper triangle"
        out.append((status[i], L, Z))
    for d in dA:
        d.free()
    for g in gL + gZ:
        if g:
            g.dev.free()
    return out, raw


def raw_slices(ns):
    """Indices of each job's words in the front end's raw status array (the layout include/xerus_amd.h documents)."""
    small = [i for i, n in enumerate(ns) if n <= 256]
    big = [i for i, n in enumerate(ns) if 256 < n <= 512]
    where = {}
    for pos, i in enumerate(small):
        where[i] = [pos]
    base = len(small)
    for pos, i in enumerate(big):
        b0 = pos // 64 * 64
        part = min(64, len(big) - b0)
        where[i] = [base + 2 * b0 + (pos - b0), base + 2 * b0 + part + (pos - b0)]
    slot = base + 2 * len(big)
    for i, n in enumerate(ns):
        if n > 512:
            blocks = (n + 255) // 256
            where[i] = list(range(slot, slot + blocks))
            slot += blocks
    return where


@functools.lru_cache(maxsize=None)
def well(n):
    return cr.well(n)


@functools.lru_cache(maxsize=None)
def graded_mats(n):
    return {name: (A, lam) for name, A, lam in cr.graded_cases(n)}


@functools.lru_cache(maxsize=None)
def failing(n, k):
    return cr.indefinite_at(n, k, 4000 + n)


def modes_of(n):
    return (0, 1, 2) if n <= 512 else (0, 1)


def measure(A, lam, shift, exp, L, Z):
    """The asserted quantities of one job whose input was A 2^exp: (res_L, res_Z, white, factor error / kappa_2)."""
    L, Z = np.ldexp(L, -exp // 2), np.ldexp(Z, exp // 2)   # exact: A 2^exp = (L 2^(exp/2)) (L 2^(exp/2))^T
    As = cr.shifted(A, shift)
    Lref, st, _ = cr.chol_ld(A, shift)
    assert st == 0
    return cr.res_L(As, L), cr.res_Z(Z, L), cr.white(As, Z), cr.factor_err(L, Lref) / cr.kappa_shifted(lam, shift)


def assert_accuracy(tag, bars, vals):
    print("%s: res_L %.2e (bar %.2e) res_Z %.2e (%.2e) white %.2e (%.2e) factor error / kappa %.2e (%.2e)"
          % (tag, vals[0], bars[0], vals[1], bars[1], vals[2], bars[2], vals[3], bars[0]))
    assert vals[0] <= bars[0], (tag, "res_L", vals[0])
    assert vals[1] <= bars[1], (tag, "res_Z", vals[1])
    assert vals[2] <= bars[2], (tag, "white", vals[2])
    assert vals[3] <= bars[0], (tag, "L against chol_ld, over kappa_2", vals[3])


# ---- (a) accuracy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.ORDERS_RR + cr.ORDERS_2X2 + cr.ORDERS_FULL)
def test_accuracy_well_conditioned(handle, n):
    """kappa = 100 at every order, every shift and both scales through the front end; the two-call form and (n <= 256,
    the same kernels) the bare batch tables must give the same bits."""
    A, lam = well(n)
    spec = cr.accuracy_jobs(n)
    jobs = [(np.ldexp(A, e), s, True, True) for s, e in spec]
    res, raw = run_jobs(handle, jobs, 0)
    assert [r[0] for r in res] == [0] * len(jobs) and not any(raw)
    bars = well_bars(n)
    for (s, e), (_, L, Z) in zip(spec, res):
        assert_accuracy("n %d shift %g scale 2^%d" % (n, s, e), bars, measure(A, lam, s, e, L, Z))
    for mode in (1, 2) if n <= 256 else (1,):
        res2, raw2 = run_jobs(handle, jobs, mode)
        assert not any(raw2)
        for (_, L, Z), (_, L2, Z2) in zip(res, res2):
            assert same(L, L2) and same(Z, Z2), "mode %d differs from mode 0" % mode


@pytest.mark.parametrize("n", cr.ORDERS_32)
def test_accuracy_32_wide_kernel(handle, n):
    """Mode 2 above 256: k_potrf32_batched and k_trinv_batched<32>."""
    A, lam = well(n)
    spec = cr.accuracy_jobs(n)
    res, raw = run_jobs(handle, [(np.ldexp(A, e), s, True, True) for s, e in spec], 2)
    assert [r[0] for r in res] == [0] * len(spec) and not any(raw)
    for (s, e), (_, L, Z) in zip(spec, res):
        assert np.array_equal(L[np.triu_indices(n, 1)], np.zeros(n * (n - 1) // 2))
        assert_accuracy("32-wide n %d shift %g scale 2^%d" % (n, s, e), well_bars(n, True), measure(A, lam, s, e, L, Z))


@pytest.mark.parametrize("n", cr.ORDERS_GRADED)
def test_accuracy_graded(handle, n):
    """Graded spectra up to the worst Gram a certificate admits (lambda_min = 4 tau tr A, factored with the shift
    -tau tr A as well)."""
    mats = graded_mats(n)
    jobs = [(mats[name][0], s, True, True) for name, s in cr.GRADED_JOBS]
    group = "rr" if n <= 256 else "b2x2" if n <= 512 else "full"
    for mode, g in ((0, group), (1, group)) + (((2, "k32"),) if 256 < n <= 512 else ()):
        res, raw = run_jobs(handle, jobs, mode)
        assert [r[0] for r in res] == [0] * len(jobs) and not any(raw)
        if mode == 1:
            assert all(same(a[1], b[1]) and same(a[2], b[2]) for a, b in zip(first, res))
            continue
        first = res
        for (name, s), (_, L, Z) in zip(cr.GRADED_JOBS, res):
            A, lam = mats[name]
            assert_accuracy("graded n %d %s shift %g mode %d" % (n, name, s, mode), BARS_GRADED[g], measure(A, lam, s, 0, L, Z))


# ---- (b) status --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.STATUS_ORDERS)
def test_status_is_one_plus_first_failing_column(handle, n):
    for k in cr.status_columns(n):
        A = failing(n, k)
        for mode in modes_of(n):
            (st, _, _), = run_jobs(handle, [(A, 0.0, True, True)], mode)[0]
            assert st == k + 1, (n, k, mode, st)
        (st, _, _), = run_jobs(handle, [(A, 0.0, False, False)], 0)[0]   # the same as a status-only job
        assert st == k + 1, (n, k, "status only", st)


@pytest.mark.parametrize("n", cr.STATUS_ORDERS)
def test_status_of_non_finite_and_zero_matrices(handle, n):
    k = n // 2
    for bad in (np.nan, np.inf, 2.0e300):
        A = well(n)[0].copy()
        A[k, k] = bad
        expect = cr.chol_ld(A)[1]
        assert expect != 0
        for mode in modes_of(n):
            (st, _, _), = run_jobs(handle, [(A, 0.0, True, True)], mode)[0]   # (returning at all is part of the test)
            assert st != 0, (n, bad, mode)
            if np.isfinite(bad):   # the pivot rule rejects >= 1e300 at exactly that column
                assert st == expect == k + 1, (n, bad, mode, st)
    for mode in modes_of(n):
        (st, _, _), = run_jobs(handle, [(np.zeros((n, n)), 0.0, True, True)], mode)[0]
        assert st == 1, (n, mode, st)


# ---- (c) certificates --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.CERT_ORDERS)
def test_certificate_on_both_sides_of_tau(handle, n):
    """lambda_min = c tau tr A: c = 0.5 must be refused (a certificate that wrongly succeeds keeps a rank the round
    should have sent to the SVD path), c = 2 must pass."""
    for c in (0.5, 2.0):
        A = cr.cert_case(n, c)
        expect = cr.chol_ld(A, -cr.TAU)[1]
        assert (expect != 0) == (c < 1.0)
        for mode in (0, 1):
            (st, _, _), = run_jobs(handle, [(A, -cr.TAU, False, False)], mode)[0]
            assert st == expect, (n, c, mode, st, expect)
        if n <= 512:   # the bare tables: status-only up to 256, with a factor above (the 32-wide kernel stores it)
            (st, _, _), = run_jobs(handle, [(A, -cr.TAU, n > 256, False)], 2)[0]
            assert st == expect, (n, c, 2, st, expect)


# ---- (d) contracts -----------------------------------------------------------------------------------------------
def nan_upper(A):
    B = A.copy()
    B[np.triu_indices(A.shape[0], 1)] = np.nan
    return B


@pytest.mark.parametrize("mode,orders", [(0, (2, 16, 17, 100, 256, 257, 300, 512, 513, 769)), (1, (17, 256, 300, 520)),
                                         (2, (2, 17, 256, 257, 300, 512))])
def test_only_the_lower_triangle_is_read(handle, mode, orders):
    """The same jobs with the strict upper triangle of A set to NaN: bit-identical results."""
    jobs = []
    for n in orders:
        jobs += [(well(n)[0], 0.0, True, True), (well(n)[0], 1.0e-9, True, False)]
        if n <= 256 or mode < 2:
            jobs.append((well(n)[0], -cr.TAU, False, False))
    res, raw = run_jobs(handle, jobs, mode)
    resn, rawn = run_jobs(handle, [(nan_upper(A), s, wl, wz) for A, s, wl, wz in jobs], mode)
    assert not any(raw) and raw == rawn
    for (A, _, _, _), a, b in zip(jobs, res, resn):
        n = A.shape[0]
        assert a[0] == b[0] == 0, (n, a[0], b[0])
        assert a[1] is None or same(a[1], b[1]), ("L", n, mode)
        assert a[2] is None or same(a[2], b[2]), ("Z", n, mode)


def potrf_solve(handle, A, shift=0.0, cols=True, Y=None, nvec=0, pad=0):
    """xrs_potrf_solve with L and X inside guard zones; ldy = ldx = natural stride + pad. Returns (status, trace, L, X)
    with X as the n x nvec solution (row tails checked to be untouched)."""
    n = A.shape[0]
    dA, gL = handle.array(A), Guarded(handle, (n, n))
    if nvec == 0:
        st, tr = handle.potrf_solve(gL.ptr, dA.ptr, n, shift)
        assert same(dA.numpy(), A)
        return st, tr, gL.get(), None
    rows, width = (n, nvec) if cols else (nvec, n)
    ld = width + pad
    Yh = np.full((rows, ld), SENTINEL)
    Yh[:, :width] = Y[:, :nvec] if cols else Y[:, :nvec].T
    dY, gX = handle.array(Yh), Guarded(handle, (rows, ld))
    st, tr = handle.potrf_solve(gL.ptr, dA.ptr, n, shift, cols, dY.ptr, ld, gX.ptr, ld, nvec)
    assert same(dA.numpy(), A) and same(dY.numpy(), Yh)
    X = gX.get()
    assert np.all(X[:, width:] == SENTINEL), "row tails of X overwritten"
    X = X[:, :width]
    return st, tr, gL.get(), (X if cols else X.T)


@pytest.mark.parametrize("n", (1, 2, 17, 100, 256, 300) + cr.ORDERS_32)
def test_potrf_contracts(handle, n):
    """potrf alone: exact zeros above the diagonal up to 512, lower triangle read, A untouched, accuracy of L."""
    A, lam = well(n)
    st, _, L, _ = potrf_solve(handle, A)
    assert st == 0
    assert np.array_equal(L[np.triu_indices(n, 1)], np.zeros(n * (n - 1) // 2))
    stn, _, Ln, _ = potrf_solve(handle, nan_upper(A))
    assert stn == 0 and same(L, Ln)
    rl = cr.res_L(cr.shifted(A, 0.0), L)
    bar = well_bars(n, n > 256)[0]
    print("potrf n %d: res_L %.2e (bar %.2e)" % (n, rl, bar))
    assert rl <= bar
    for k in sorted({0, n // 2, n - 1}):
        assert potrf_solve(handle, failing(n, k))[0] == k + 1


# ---- (e) batching ------------------------------------------------------------------------------------------------
_alone = {}


def alone(handle, key, job):
    """The job run as the only one of a mode-0 call (cached by key)."""
    if key not in _alone:
        (res,), raw = run_jobs(handle, [job], 0)
        _alone[key] = res
    return _alone[key]


def small_list():
    """100 jobs of n <= 256, orders cycling; failing jobs at 0, 47, 48 and 99."""
    out = []
    for i in range(100):
        n = cr.ORDERS_RR[i % len(cr.ORDERS_RR)]
        if i in (0, 47, 48, 99):
            n = max(n, 2)
            out.append((("fail", n, n // 2), (failing(n, n // 2), 0.0, True, True)))
        else:
            out.append((("well", n), (well(n)[0], 0.0, True, True)))
    return out


def big_list():
    """66 jobs of 257..260 and one each of 300, 511, 512; failing at 0, 63, 64 and 68, in different halves."""
    ns = [257 + i % 4 for i in range(66)] + [300, 511, 512]
    fail = {0: 10, 63: 256, 64: 255, 68: 511}
    out = []
    for i, n in enumerate(ns):
        if i in fail:
            out.append((("fail", n, fail[i]), (failing(n, fail[i]), 0.0, True, True)))
        else:
            out.append((("well", n), (well(n)[0], 0.0, True, True)))
    return out


def full_list():
    """Three chol_full jobs, the middle one failing in block 1."""
    return [(("well", 513), (well(513)[0], 0.0, True, True)), (("fail", 520, 300), (failing(520, 300), 0.0, True, True)),
            (("well", 520), (well(520)[0], 0.0, True, True))]


def kinds_list():
    """Factor jobs, Z-less factor jobs and certificates mixed, over the three size classes."""
    out = []
    for i, n in enumerate((17, 100, 256, 300, 33, 513, 257, 48, 129, 512, 16, 241)):
        A = well(n)[0]
        kind = i % 3
        if kind == 0:
            out.append((("well", n), (A, 0.0, True, True)))
        elif kind == 1:
            out.append((("noz", n), (A, 0.0, True, False)))
        else:
            out.append((("cert", n), (A, -cr.TAU, False, False)))
    out.insert(5, (("certfail", 100), (failing(100, 50), -cr.TAU, False, False)))
    return out


def check_batch(handle, keyed):
    ns = [job[0].shape[0] for _, job in keyed]
    where = raw_slices(ns)
    single = [alone(handle, key, job) for key, job in keyed]
    res0, raw0 = run_jobs(handle, [job for _, job in keyed], 0)
    res1, raw1 = run_jobs(handle, [job for _, job in keyed], 1)
    assert len(raw0) == len(raw1) == sum(len(w) for w in where.values())
    for i, ((key, _), s, r0, r1) in enumerate(zip(keyed, single, res0, res1)):
        assert r0[0] == r1[0] == s[0], (i, key, r0[0], r1[0], s[0])
        assert (s[0] != 0) == key[0].endswith("fail"), (i, key, s[0])
        if key[0] == "fail":
            assert s[0] == key[2] + 1, (i, key, s[0])
        if s[0] == 0:
            assert all(raw0[w] == 0 and raw1[w] == 0 for w in where[i]), (i, key, [raw0[w] for w in where[i]])
            for which in (1, 2):
                if s[which] is not None:
                    assert same(r0[which], s[which]), (i, key, "LZ"[which - 1], "batched differs from alone")
                    assert same(r1[which], r0[which]), (i, key, "LZ"[which - 1], "mode 1 differs from mode 0")
        else:
            assert any(raw0[w] != 0 for w in where[i])


def test_batch_of_100_small_jobs(handle):
    check_batch(handle, small_list())


def test_batch_of_69_two_by_two_jobs(handle):
    check_batch(handle, big_list())


def test_batch_of_full_jobs(handle):
    check_batch(handle, full_list())


def test_batch_of_every_class_mixed(handle):
    s, b, f = small_list(), big_list(), full_list()
    mixed = []
    for i in range(max(len(s), len(b))):   # interleaved, so that job order and status layout differ
        mixed += s[i:i + 1] + b[i:i + 1] + f[i:i + 1]
    check_batch(handle, mixed)


def test_batch_of_mixed_job_kinds(handle):
    check_batch(handle, kinds_list())


def test_bare_tables_split_small_and_large(handle):
    """Mode 2: 48 entries mixing n <= 256 and n > 256 (the small / large split and slot mapping of potrf_batched, the
    two launches of trinv_batched), failing entries of both kinds among them."""
    ns = [(17, 300, 100, 257, 256, 512, 1, 289)[i % 8] for i in range(48)]
    fail = {0: 8, 5: 400, 20: 50, 47: 288}   # index -> failing column (orders 17, 512, 256, 289)
    jobs = [(failing(n, fail[i]) if i in fail else well(n)[0], 0.0, True, i % 3 != 1) for i, n in enumerate(ns)]
    res, raw = run_jobs(handle, jobs, 2)
    assert raw == [r[0] for r in res]
    for i, (n, job, r) in enumerate(zip(ns, jobs, res)):
        assert r[0] == (fail[i] + 1 if i in fail else 0), (i, n, r[0])
        if i in fail:
            continue
        key = ("bare", n, job[3])
        if key not in _alone:
            _alone[key] = run_jobs(handle, [job], 2)[0][0]
        assert same(r[1], _alone[key][1]) and (r[2] is None or same(r[2], _alone[key][2])), (i, n)
        if n <= 256:   # the same kernels as the front end's
            s = alone(handle, ("well", n), (well(n)[0], 0.0, True, True))
            assert same(r[1], s[1]) and (r[2] is None or same(r[2], s[2])), (i, n)


# ---- (f) trsm and the trace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.TRSM_ORDERS)
def test_trsm_and_trace(handle, n):
    """X = L^{-1} Y against a long-double forward substitution with the device's own L, columns and rows, natural and
    padded strides; info[0] against the diagonal sum."""
    A, _ = well(n)
    Y = cr.rhs(n)
    bar = BARS_TRSM[next(g for g, orders in cr.TRSM_GROUPS.items() if n in orders)]
    Lfirst, Xref, worst = None, None, 0.0
    for nvec in cr.TRSM_NVEC:
        for cols in (True, False):
            for pad in (0, 3):
                st, tr, L, X = potrf_solve(handle, A, 0.0, cols, Y, nvec, pad)
                assert st == 0
                assert abs(tr - float(A.diagonal().astype(cr.LD).sum())) <= 4 * n * cr.U * np.abs(A.diagonal()).sum()
                if Lfirst is None:
                    Lfirst, Xref = L, cr.forward_ld(L, Y)
                assert same(L, Lfirst)
                err = cr.factor_err(X, Xref[:, :nvec])
                worst = max(worst, err)
                assert err <= bar, (n, nvec, cols, pad, err, bar)
    print("trsm n %d: worst error %.2e (bar %.2e)" % (n, worst, bar))
