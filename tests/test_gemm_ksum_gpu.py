"""GPU: xrs_gemm_ksum (gemm_ksum.hip), C = alpha sum_j A_j B_j over operands in different allocations, against
NumPy's sum of A_j @ B_j.

Tolerance, elementwise: 4 (sum K + count) u (sum_j |A_j| |B_j|) with u = 2^-53 -- the standard bound of a dot product
of sum K terms summed in any order, plus one rounding per combined partial sum, for the kernel and for NumPy each;
derived, not tuned. A call with sum K = 0 must give exact zeros."""
import numpy as np
import pytest

from xerus_amd import capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ALPHA = -0.75
SHAPES = [(1, 1), (16, 16), (37, 19), (65, 130)]
KSET = [0, 1, 3, 4, 17, 130]
TABLE = 32                      # segments per launch (kKsumTable)
COUNTS = [1, 2, 5, TABLE + 1]   # the last: one past a full table, so a second launch


def _ks(count, shift):
    return [KSET[(j + shift) % len(KSET)] for j in range(count)]


def _operands(rng, M, N, Ks):
    return [rng.standard_normal((M, k)) for k in Ks], [rng.standard_normal((k, N)) for k in Ks]


def _expect(As, Bs, M, N):
    ref, mag = np.zeros((M, N)), np.zeros((M, N))
    for a, b in zip(As, Bs):
        ref += a @ b
        mag += np.abs(a) @ np.abs(b)
    return ALPHA * ref, mag


def _check(got, As, Bs, M, N, what):
    ref, mag = _expect(As, Bs, M, N)
    ktot = sum(a.shape[1] for a in As)
    tol = 4 * (ktot + len(As)) * U * mag
    err = np.abs(got - ref)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / tol {worst:.3f}")
    assert np.all(err <= tol), (what, float(err.max()))


def _view(handle, a, pad):
    """a as a view into a larger buffer: row stride a.shape[1] + pad, base pointer one double past the allocation's."""
    rows, cols = a.shape
    ld = cols + pad
    host = np.full(1 + rows * ld, np.nan)   # what a kernel must never read or may read only as padding
    host[1:].reshape(rows, ld)[:, :cols] = a
    base = handle.array(host)
    return base, capi.DeviceArray(handle, (rows, cols), ptr=base.ptr + 8, owned=False), ld


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_case_matrix(handle, si, count):
    M, N = SHAPES[si]
    Ks = _ks(count, si)
    rng = np.random.default_rng(100 * si + count)
    As, Bs = _operands(rng, M, N, Ks)
    out = handle.empty((M, N))
    handle.gemm_ksum(out, M, N, ALPHA, [handle.array(a) for a in As], [handle.array(b) for b in Bs], Ks)
    _check(out.numpy(), As, Bs, M, N, f"{M}x{N} count {count} K {Ks[:6]}")


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_case_matrix_on_views(handle, si, count):
    """lda_j > K_j, ldb_j > N, base pointers offset by one double; the padding is NaN, so a read of it shows."""
    M, N = SHAPES[si]
    Ks = _ks(count, si + 1)
    rng = np.random.default_rng(1000 + 100 * si + count)
    As, Bs = _operands(rng, M, N, Ks)
    va = [_view(handle, a, 3) for a in As]
    vb = [_view(handle, b, 5) for b in Bs]
    out = handle.empty((M, N))
    handle.gemm_ksum(out, M, N, ALPHA, [v[1] for v in va], [v[1] for v in vb], Ks, [v[2] for v in va], [v[2] for v in vb])
    _check(out.numpy(), As, Bs, M, N, f"views {M}x{N} count {count} K {Ks[:6]}")


def test_sliced_path_and_reproducibility(handle):
    """M = N = 16, 8 segments of K = 512: one tile, 256 chunks, so the concatenated K is cut into slices whose slabs
    the combine kernel sums (one GEMM launch + one combine launch). Same bound; two calls give identical bits."""
    M = N = 16
    Ks = [512] * 8
    As, Bs = _operands(np.random.default_rng(77), M, N, Ks)
    dA, dB = [handle.array(a) for a in As], [handle.array(b) for b in Bs]
    out1, out2 = handle.empty((M, N)), handle.empty((M, N))
    handle.prof_begin(capi.KFAM_GEMM | capi.KFAM_SPLITK)
    handle.gemm_ksum(out1, M, N, ALPHA, dA, dB)
    prof = handle.prof_end()
    assert prof["launches"] == 2, prof
    handle.gemm_ksum(out2, M, N, ALPHA, dA, dB)
    a, b = out1.numpy(), out2.numpy()
    _check(a, As, Bs, M, N, "sliced 16x16, 8 x K 512")
    assert np.array_equal(a, b)


def test_empty_segments(handle):
    """K_j = 0 contributes nothing and its pointers are not looked at (null is accepted); all segments empty: C = 0."""
    M, N = 37, 19
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((M, 17)), rng.standard_normal((17, N))
    out = handle.array(np.full((M, N), np.nan))
    handle.gemm_ksum(out, M, N, ALPHA, [None, handle.array(a), None], [None, handle.array(b), None], [0, 17, 0], [1, 17, 1])
    _check(out.numpy(), [a], [b], M, N, "null pointers at K = 0")
    handle.gemm_ksum(out, M, N, ALPHA, [None], [None], [0], [1])
    assert np.array_equal(out.numpy(), np.zeros((M, N)))


def test_argument_errors(handle):
    a, b = handle.array(np.ones((16, 16))), handle.array(np.ones((16, 16)))
    out = handle.empty((16, 16))
    for args in [
        (out, 16, 16, 1.0, [None], [b], [16], [16]),           # null A with K > 0
        (out, 16, 16, 1.0, [a], [None], [16], [16]),           # null B with K > 0
        (out, 16, 16, 1.0, [], [], [], []),                    # count = 0
        (a, 16, 16, 1.0, [a], [b], [16], [16]),                # C aliases A
        (b, 16, 16, 1.0, [a], [b], [16], [16]),                # C aliases B
        (out, 16, 16, 1.0, [a], [b], [16], [8]),               # lda < K
        (out, 16, 16, 1.0, [a], [b], [16], [16], [8]),         # ldb < N
        (out, 0, 16, 1.0, [a], [b], [16], [16]),               # M = 0
    ]:
        with pytest.raises(capi.XrsError) as e:
            handle.gemm_ksum(*args)
        assert e.value.code == -1
    # a view one double into C's allocation aliases C too
    inner = capi.DeviceArray(handle, (8, 16), ptr=out.ptr + 8, owned=False)
    with pytest.raises(capi.XrsError):
        handle.gemm_ksum(out, 16, 16, 1.0, [a], [inner], [8], [16])
