"""GPU: find_largest_entry and what it stands on -- the symmetric-square kernel (xrs_tt_entrywise_square), the
rank-one argmax (xrs_tt_rank_one_argmax), TTTensor.__getitem__ and xe.entrywise_square -- against the closed
forms and the fixtures of tests/largest_entry_ref.py (reference: src/xerus/algorithms/largestEntry.cpp:6-54,
unit test src/unitTests/largestEntry.cxx:28-76)."""
import numpy as np
import pytest

import largest_entry_ref as ler
from xerus_amd import capi

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52


def _random_cores(ranks, ext, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((ranks[k], ext[k], ranks[k + 1])) for k in range(len(ext))]


# ------------------------------------------------------------------------------------------ symmetric square
SQUARE_CASES = [
    ((1, 3, 4, 2, 1), (3, 4, 2, 3), 1.0),
    ((1, 2, 1, 3, 1), (2, 3, 2, 2), 1.0),      # an interior rank 1
    ((1, 17, 17, 1), (2, 3, 2), 1.0),          # s = 153: the right pair index crosses wave and workgroup boundaries
    ((1, 2, 3, 1), (3, 1, 2), 1.0),            # a mode of size 1
    ((1, 1), (5,), 1.0),                       # d = 1
    ((1, 3, 4, 2, 1), (3, 4, 2, 3), -0.5),     # alpha into the first core
]


@pytest.mark.parametrize("ranks,ext,alpha", SQUARE_CASES)
def test_symmetric_square_kernel_vs_closed_form(handle, ranks, ext, alpha):
    """Every entry within 4 * 2^-52 of the closed form, relative to the largest product of two core entries
    involved; the a = b, a' = b' entries bit-equal to A * A; r_out = r (r + 1) / 2."""
    cores = _random_cores(ranks, ext, 11 * len(ext) + ranks[1])
    x = capi.TTDevice.from_cores(handle, cores)
    z = x.entrywise_square(alpha)
    assert z.r == [ler.sym_rank(r) for r in ranks]
    assert z.dims == list(ext)
    got = z.cores()
    for k, A in enumerate(cores):
        f = alpha if k == 0 else 1.0
        want = f * ler.symmetric_square_core(A)
        scale = abs(f) * ler.symmetric_square_scale(A)
        err = np.abs(got[k] - want)
        worst = float(np.max(err / np.maximum(scale, 1e-300)))
        print("core", k, "max error / scale = %.3g ulp" % (worst / ULP))
        assert np.all(err <= 4 * ULP * scale), (k, worst / ULP)
        ra, rb = A.shape[0], A.shape[2]
        diag_l = [ler.pair_index(a, a, ra) for a in range(ra)]
        diag_r = [ler.pair_index(a, a, rb) for a in range(rb)]
        assert np.array_equal(got[k][np.ix_(diag_l, range(A.shape[1]), diag_r)], f * (A * A))
    z.free()
    x.free()


def test_symmetric_square_kernel_rejects_bad_arguments(handle):
    """The error conventions of xrs_tt_entrywise_product: boundary ranks must be 1."""
    cores = _random_cores((2, 2, 1), (2, 2), 3)
    x = capi.TTDevice.from_cores(handle, cores)
    with pytest.raises(capi.XrsError):
        x.entrywise_square()
    x.free()


def _dense(xe, t):
    return xe.Tensor(t).to_ndarray()


def test_entrywise_square_tttensor(xe):
    xe.seed(0xBAADF00D)
    A = xe.TTTensor.random([2, 3, 2, 3, 2, 3], [3, 4, 4, 3, 2])
    A.move_core(3)
    f = _dense(xe, A)
    S = xe.entrywise_square(A)
    assert np.linalg.norm(_dense(xe, S) - f * f) / np.linalg.norm(f * f) < 1e-13
    assert S.canonicalized and S.corePosition == 3
    # the Kronecker form stays what it was and represents the same tensor
    K = xe.entrywise_product(A, A)
    assert np.linalg.norm(_dense(xe, K) - f * f) / np.linalg.norm(f * f) < 1e-13
    # not canonical: no move, the ranks are s(r)
    R = xe.TTTensor.random_raw([4, 4, 4, 4], [3, 4, 3])
    assert not R.canonicalized
    SR = xe.entrywise_square(R)
    assert not SR.canonicalized
    assert SR.ranks() == [6, 10, 6]
    g = _dense(xe, R)
    assert np.linalg.norm(_dense(xe, SR) - g * g) / np.linalg.norm(g * g) < 1e-13
    # a pending factor on a component is squared
    R2 = R * 3.0
    assert np.linalg.norm(_dense(xe, xe.entrywise_square(R2)) - 9.0 * g * g) / np.linalg.norm(9.0 * g * g) < 1e-13


def test_entrywise_square_ttoperator(xe):
    xe.seed(0xBAADF00D)
    A = xe.TTOperator.random([2, 3, 2, 3, 2, 2], [3, 3])
    A.move_core(1)
    f = _dense(xe, A)
    S = xe.entrywise_square(A)
    assert S.dimensions == [2, 3, 2, 3, 2, 2]
    assert np.linalg.norm(_dense(xe, S) - f * f) / np.linalg.norm(f * f) < 1e-13
    assert S.canonicalized and S.corePosition == 1


# ------------------------------------------------------------------------------------------ rank-one argmax
def test_rank_one_argmax(handle):
    big = np.linspace(-1.0, 1.0, 300)
    big[10], big[270] = 5.0, -5.0                 # more than one pass of the workgroup; a tie across passes
    late = np.zeros(300)
    late[299] = -1e-3                             # the winner in the second pass only
    with_nan = np.array([np.nan, 1.0, -2.0, np.nan])
    vectors = [
        np.array([1.0, -2.0, 2.0, 0.5]),          # a tie: the first index wins; the largest entry is negative
        np.array([0.25]),                         # a mode of size 1
        big,
        late,
        np.arange(12.0).reshape(3, 4) - 3.0,      # operator-style ext n m = 3 * 4: 8 at (2, 3)
        with_nan,                                 # NaN never wins
        np.zeros(5),                              # all equal: index 0
    ]
    x = capi.TTDevice.from_cores(handle, [v.reshape(1, -1, 1) for v in vectors])
    assert x.rank_one_argmax() == [1, 0, 10, 299, 11, 2, 0]
    x.free()
    y = capi.TTDevice.from_cores(handle, _random_cores((1, 2, 1), (2, 2), 5))
    with pytest.raises(ValueError):
        y.rank_one_argmax()
    y.free()


# ------------------------------------------------------------------------------------------ operator[]
def test_tttensor_getitem(xe):
    xe.seed(0xBAADF00D)
    dims = [3, 4, 2, 5, 3]
    A = xe.TTTensor.random(dims, [3, 4, 4, 2]) * 1.5
    f = _dense(xe, A)
    tol = 1e-13 * np.max(np.abs(f))
    rng = np.random.default_rng(9)
    for p in rng.integers(0, f.size, 50):
        idx = [int(i) for i in np.unravel_index(int(p), dims)]
        assert abs(A[int(p)] - f.ravel()[p]) <= tol
        assert abs(A[idx] - f[tuple(idx)]) <= tol
    assert abs(A[f.size - 1] - f.ravel()[-1]) <= tol
    with pytest.raises(RuntimeError):
        A[f.size]
    with pytest.raises(RuntimeError):
        A[[0, 4, 0, 0, 0]]
    with pytest.raises(RuntimeError):
        A[[0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------ find_largest_entry
@pytest.fixture(scope="module")
def fixtures():
    out = []
    for dims, ranks, seed in ler.FIXTURES:
        x = ler.make_fixture(dims, ranks, seed)
        out.append((x, x.full()))
    return out


def _upload(xe, x, sign=1.0):
    """The TTTensor with the oracle's cores (core at 0, as TT.random leaves it)."""
    t = xe.TTTensor(x.dims)
    for k, c in enumerate(x.cores):
        t.set_component(k, xe.Tensor.from_ndarray(sign * c if k == 0 else c))
    t.assume_core_position(0)
    return t


@pytest.mark.parametrize("case", range(len(ler.FIXTURES)), ids=ler.FIXTURE_IDS)
def test_find_largest_entry_fixtures(xe, fixtures, case):
    """The position is the brute-force argmax of |dense|; also for the sign-flipped tensor; the input is unchanged."""
    x, full = fixtures[case]
    pos, largest, alpha = ler.gap(full)
    t = _upload(xe, x)
    got = xe.find_largest_entry(t, alpha, abs(largest))
    print("position", got, "expected", pos, "alpha %.4f" % alpha, "largest %.6g" % largest)
    assert got == pos
    for k, c in enumerate(x.cores):
        assert np.array_equal(t.get_component(k).to_ndarray(), c)
    assert t.canonicalized and t.corePosition == 0
    assert abs(t[got] - largest) <= 1e-13 * abs(largest)
    flipped = _upload(xe, x, -1.0)
    assert xe.find_largest_entry(flipped, alpha, abs(largest)) == pos


def test_find_largest_entry_ttoperator(xe):
    """Dimensions [2,3,2, 3,2,2], rank 3: a rank-2 operator plus a planted entry twice as large as any other.
    The position is row-major in the operator's own order (i_0..i_2, j_0..j_2)."""
    dims = [2, 3, 2, 3, 2, 2]
    rng = np.random.default_rng(21)
    merged = [rng.standard_normal(s) for s in ((1, 6, 2), (2, 6, 2), (2, 4, 1))]
    full = np.einsum('xay,ybz,zcw->abc', *merged).reshape(2, 3, 3, 2, 2, 2).transpose(0, 2, 4, 1, 3, 5)
    idx = (1, 2, 0, 2, 0, 1)
    full = np.ascontiguousarray(full)
    full[idx] = 0.0
    planted = -2.0 * np.max(np.abs(full))
    full[idx] = planted
    pos, largest, alpha = ler.gap(full)
    assert alpha <= 0.5 and largest == planted and pos == int(np.ravel_multi_index(idx, dims))
    op = xe.TTOperator(xe.Tensor.from_ndarray(full))
    assert op.ranks() == [3, 3]
    got = xe.find_largest_entry(op, alpha, abs(largest))
    assert got == pos
    assert abs(xe.Tensor(op)[got] - planted) <= 1e-12 * abs(planted)


def test_find_largest_entry_guard(xe):
    """A TT with a NaN entry raises instead of looping."""
    x = ler.make_fixture([3, 2, 3, 2], [3, 3, 3], 1)
    x.cores[2][1, 0, 1] = np.nan
    t = xe.TTTensor(x.dims)
    for k, c in enumerate(x.cores):
        t.set_component(k, xe.Tensor.from_ndarray(c))
    with pytest.raises(RuntimeError):
        xe.find_largest_entry(t, 0.9, 0.0)
