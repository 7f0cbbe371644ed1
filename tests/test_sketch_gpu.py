"""GPU: the counter-based Gaussian matrix G(seed, stream) and the sketch Y = G A (xrs_philox_words,
xrs_gaussian_matrix, xrs_sketch_gaussian; csrc/philox.hpp, csrc/sketch.hip) against the NumPy
restatement of tests/random_ttsvd_ref.py."""
import numpy as np
import pytest

import random_ttsvd_ref as rr
from xerus_amd import capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# workgroups of the fused kernel split m into slabs of at least 256 rows: 1061 rows are five slabs, the last one
# ragged (37 rows: two 16-row chunks and a masked third)
MULTI_SLAB = (40, 1061, 16)


# ------------------------------------------------------------------------------------------ words and normals
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 12345])
@pytest.mark.parametrize("stream", [0, 7])
def test_philox_words_bit_exact(handle, seed, stream):
    """The device words equal the NumPy Philox4x32-10 bit for bit. The carry of the block index q into the second
    counter word needs q >= 2^32, i.e. 2^34 columns: out of reach at test size, so `q high` is only ever 0 here."""
    got = handle.philox_words(3, 5, seed, stream)
    assert got.shape == (3, 5, 4) and got.dtype == np.uint32
    assert np.array_equal(got, rr.words(seed, stream, 3, 5))


def test_gaussian_matrix_follows_the_formula(handle):
    """A mapping check, not an accuracy claim: a wrong word, pair or position is an O(1) difference, the fp32
    intrinsics of the device are about 1e-6 from the fp64 formula."""
    seed, stream, s, m = 0x0123456789ABCDEF, 3, 33, 1030   # m = 2 mod 4: a masked word block at every row end
    got = handle.gaussian_matrix(s, m, seed, stream).numpy()
    want = rr.gaussian_matrix(seed, stream, s, m)
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("max |dG| / max(1, |G|) = %.3e over %d normals" % (dev.max(), dev.size))
    assert np.all(np.isfinite(got))
    assert dev.max() <= 1e-3


def test_prefix_property_bit_exact(handle):
    big = handle.gaussian_matrix(17, 130, 99, 4).numpy()
    small = handle.gaussian_matrix(5, 37, 99, 4).numpy()
    assert np.array_equal(small, big[:5, :37])
    assert not np.array_equal(handle.gaussian_matrix(5, 37, 99, 5).numpy(), small)    # another stream
    assert not np.array_equal(handle.gaussian_matrix(5, 37, 100, 4).numpy(), small)   # another seed


# ------------------------------------------------------------------------------------------ the product
# s in {1, 5, 16, 17, 40}, m in {1, 3, 64, 257, 4099}, n in {1, 7, 16, 33, 300}: every value with several partners
COVER = [
    (1, 1, 1), (1, 64, 16), (1, 4099, 7), (1, 257, 300),
    (5, 3, 7), (5, 64, 1), (5, 257, 33), (5, 4099, 16),
    (16, 1, 16), (16, 3, 300), (16, 64, 33), (16, 257, 7), (16, 4099, 1),
    (17, 1, 33), (17, 3, 1), (17, 64, 300), (17, 257, 16), (17, 4099, 7),
    (40, 1, 7), (40, 3, 16), (40, 64, 300), (40, 257, 1), (40, 4099, 33),
]
# the remaining instances of the fused kernel (4 and 5 row blocks: 49 <= s <= 80) and the slab case
PATHS = [(64, 300, 16), (64, 257, 33), (72, 805, 16), (80, 64, 40), MULTI_SLAB]


def _check_product(handle, s, m, n, route, A=None, dA=None, out=None):
    seed, stream = 7 * s + m, n % 5
    if A is None:
        A = np.random.default_rng(s * 10007 + m * 31 + n).standard_normal((m, n))
        dA = handle.array(A)
    G = handle.gaussian_matrix(s, m, seed, stream).numpy()
    Y = handle.sketch_gaussian(s, dA, seed, stream, route=route, m=m, out=out)
    assert handle.sketch_last_route() == {1: "fused", 2: "materialised"}[route]
    got = Y.numpy().ravel()[:s * n].reshape(s, n)
    want = np.asarray(G.astype(np.longdouble) @ A[:m].astype(np.longdouble), dtype=np.float64)
    bound = 2 * m * U * (np.abs(G) @ np.abs(A[:m]))
    err = np.abs(got - want)
    print("(%d, %d, %d) route %d: max error / bound = %.3g" % (s, m, n, route, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(np.isfinite(got))
    assert np.all(err <= bound)
    return got


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("s,m,n", COVER + PATHS)
def test_sketch_product(handle, s, m, n, route):
    """|Y - G A| <= 2 m 2^-53 (|G| |A|) elementwise, G downloaded from xrs_gaussian_matrix: the fp64 dot-product
    bound with a factor 2 for the split's reordering. Both routes; the handle reports the route that ran."""
    _check_product(handle, s, m, n, route)


@pytest.mark.parametrize("s,m,n", [(17, 257, 33), (5, 3, 7)])
@pytest.mark.parametrize("route", [1, 2])
def test_sketch_stays_inside_its_buffers(handle, s, m, n, route):
    """A is the first m rows of a larger array whose other rows are NaN, Y the first s n doubles of a larger array
    filled with a sentinel: the result is finite and within the bound, the sentinel intact."""
    rng = np.random.default_rng(5)
    A = np.full((m + 70, n), np.nan)
    A[:m] = rng.standard_normal((m, n))
    sentinel = -777.25
    out = handle.array(np.full(s * n + 4096, sentinel))
    _check_product(handle, s, m, n, route, A=A, dA=handle.array(A), out=out)
    assert np.all(out.numpy()[s * n:] == sentinel)


def test_fused_sketch_is_reproducible(handle):
    s, m, n = MULTI_SLAB
    dA = handle.array(np.random.default_rng(1).standard_normal((m, n)))
    first = handle.sketch_gaussian(s, dA, 42, 1, route=1).numpy()
    second = handle.sketch_gaussian(s, dA, 42, 1, route=1).numpy()
    assert np.array_equal(first, second)


def test_auto_route_runs_one_of_the_two(handle):
    dA = handle.array(np.random.default_rng(2).standard_normal((300, 16)))
    auto = handle.sketch_gaussian(24, dA, 9, 2).numpy()
    route = handle.sketch_last_route()
    assert route in ("fused", "materialised")
    forced = handle.sketch_gaussian(24, dA, 9, 2, route={"fused": 1, "materialised": 2}[route]).numpy()
    assert np.array_equal(auto, forced)
    # outside the fused envelope (s > 80) the automatic choice is the materialised route
    handle.sketch_gaussian(81, dA, 9, 2)
    assert handle.sketch_last_route() == "materialised"


def test_sketch_rejects_bad_arguments(handle):
    """XRS_EINVAL -> capi.XrsError: empty shapes, a row or stream index of 2^32 or more, an unknown route, the
    fused route asked for more rows than it holds."""
    dA = handle.array(np.ones((4, 3)))
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(0, dA, 1)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(2, dA, 1, m=0)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(2, capi.DeviceArray(handle, (4, 0)), 1)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(2 ** 32 + 1, dA, 1)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(2, dA, 1, stream=2 ** 32)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(2, dA, 1, route=3)
    with pytest.raises(capi.XrsError):
        handle.sketch_gaussian(81, dA, 1, route=1)
    for fn in (handle.gaussian_matrix, handle.philox_words):
        with pytest.raises(capi.XrsError):
            fn(0, 4, 1)
        with pytest.raises(capi.XrsError):
            fn(4, 0, 1)
        with pytest.raises(capi.XrsError):
            fn(2 ** 32 + 1, 1, 1)
        with pytest.raises(capi.XrsError):
            fn(2, 2, 1, 2 ** 32)
    assert handle.sketch_gaussian(2, dA, 1).numpy().shape == (2, 3)   # the handle is still usable
