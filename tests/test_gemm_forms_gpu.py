"""The fp64 GEMM family (xrs_gemm, xrs_gemm_batched, xrs_gemm_sym and the internal forms behind xrs_gemm_forms) at
the operand forms the shape tests never reach: leading dimensions larger than the row length, operands 8 B off
16-B alignment, a batch with one misaligned entry, triangular skipping and the symmetric batch.

Every operand lies inside a NaN-filled buffer (its ld padding, the doubles before it and 64 doubles after it are
NaN), so a load outside rows x rowlen that reaches the product shows as a non-finite result; every C lies between
two 64-double guard bands of a sentinel that must stay bit-intact.

Measure, per element: with want = alpha (op(A) op(B)) evaluated in long double and rounded to double,
    |got - want| <= (K + 3) 2^-53 |alpha| (|op(A)| |op(B)|).
This is the fp64 dot-product bound for ANY summation order with fused multiply-adds (K roundings: it covers split-K
slices and the wave-group reductions), plus one rounding for the alpha multiply and two for the reference (its
long-double evaluation and its rounding to double). Derived, not tuned. Where the bound is 0 the result must be an
exact 0. Each case prints max(err / bound).

Symmetric products of the form X^T (G_s X): B = G_s X is rounded, so the product of the operands as given is
symmetric only up to that rounding, while the kernel computes the elements on or below the diagonal and mirrors
them. The bound is therefore checked for the lower triangle against the reference and for the upper triangle
against the reference's transpose (the values the kernel mirrors); with A = B = X the full matrix is checked.
"""
import functools

import numpy as np
import pytest

from xerus_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 64
ALPHA = -1.75
U = 2.0 ** -53
PAIRS = [(False, False), (False, True), (True, False), (True, True)]
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs a long double wider than fp64"


def embed(handle, mat, ld, off):
    """`mat` at element offset `off` with leading dimension `ld` inside a NaN-filled device buffer of
    off + rows ld + 64 doubles: (view of the operand, the buffer that owns the memory)."""
    rows, rowlen = mat.shape
    assert ld >= rowlen
    host = np.full(off + rows * ld + 64, np.nan)
    host[off:off + rows * ld].reshape(rows, ld)[:, :rowlen] = mat
    base = handle.array(host)
    assert base.ptr % 16 == 0
    view = capi.DeviceArray(handle, (rows, ld), ptr=base.ptr + 8 * off, owned=False)
    return view, base


class Guarded:
    """An M x N result at element offset 64 of a sentinel-filled buffer with 64 guard doubles on each side."""

    def __init__(self, handle, M, N):
        self.M, self.N = M, N
        self.base = handle.array(np.full(2 * GUARD + M * N, SENTINEL))
        self.view = capi.DeviceArray(handle, (M, N), ptr=self.base.ptr + 8 * GUARD, owned=False)

    def result(self):
        host = self.base.numpy()
        guard = np.full(GUARD, SENTINEL)
        assert np.array_equal(host[:GUARD], guard), "guard below C overwritten"
        assert np.array_equal(host[GUARD + self.M * self.N:], guard), "guard above C overwritten"
        return host[GUARD:GUARD + self.M * self.N].reshape(self.M, self.N).copy()


def shape_of(rows, K, t):
    """Stored shape of A (rows = M, t = ta) or of B (rows = N, t = not tb)."""
    return (K, rows) if t else (rows, K)


def reference(A, ta, B, tb, alpha=ALPHA):
    """(want, bound) of alpha op(A) op(B): the long-double product rounded to double and the elementwise bound."""
    opA = (A.T if ta else A).astype(LD)
    opB = (B.T if tb else B).astype(LD)
    K = opA.shape[1]
    want = (LD(alpha) * (opA @ opB)).astype(np.float64)
    bound = LD(K + 3) * LD(U) * LD(abs(alpha)) * (np.abs(opA) @ np.abs(opB))
    return want, bound


def check(got, want, bound, label, factor=1):
    """got within factor x bound of want in every element, finite, exact zeros where the bound is 0."""
    assert got.shape == want.shape
    assert np.all(np.isfinite(got)), "%s: non-finite result" % label
    err = np.abs(got.astype(LD) - want.astype(LD))
    zero = bound == 0
    assert np.all(got[zero] == 0.0), "%s: nonzero result where the bound is 0" % label
    ratio = float(np.max(np.where(zero, 0.0, err / np.where(zero, 1.0, bound)))) if got.size else 0.0
    print("%s: max(err / bound) = %.3g" % (label, ratio))
    bad = np.argwhere(err > factor * bound)
    assert bad.size == 0, "%s: %d elements outside %d x bound, first %s, max ratio %.3g" % (
        label, len(bad), factor, bad[0], ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def operands(M, N, K, ta, tb, seed):
    """The seeded operands of a case with their reference, computed once and never modified."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal(shape_of(M, K, ta))
    B = rng.standard_normal(shape_of(N, K, not tb))
    want, bound = reference(A, ta, B, tb)
    for x in (A, B, want, bound):
        x.setflags(write=False)
    return A, B, want, bound


def run_gemm(handle, M, N, K, ta, tb, A, B, lda, ldb, offa, offb, alpha=ALPHA):
    dA, keepA = embed(handle, A, lda, offa)
    dB, keepB = embed(handle, B, ldb, offb)
    out = Guarded(handle, M, N)
    handle.gemm(out.view, M, N, alpha, dA, lda, ta, K, dB, ldb, tb)
    return out.result()


def rowlens(M, N, K, ta, tb):
    return (M if ta else K), (K if tb else N)


# ------------------------------------------------------------------ 1 / 2: the LDS-DMA pipeline gate, both sides
# whole-tile shapes: 64x64 tiles with one K slice; with two slices (in-launch ticket combine); 32x32 tiles; 64x64
GATE_SHAPES = [(64, 64, 64), (64, 64, 256), (32, 96, 32), (64, 128, 64)]


def gate_variant(M, N, K, ta, tb, which):
    """(lda, ldb, offa, offb): 'in' = padded even ld at a 16-B aligned start (the pipeline's gate holds); 'lda' /
    'ldb' = that ld odd; 'ptr' = A 8 B off 16-B alignment (each leaves the gate on a whole-tile shape)."""
    ra, rb = rowlens(M, N, K, ta, tb)
    lda, ldb, offa, offb = ra + 2, rb + 6, 2, 2
    if which == "lda":
        lda = ra + 1
    elif which == "ldb":
        ldb = rb + 1
    elif which == "ptr":
        offa = 1
    return lda, ldb, offa, offb


@pytest.mark.parametrize("ta,tb", PAIRS)
@pytest.mark.parametrize("M,N,K", GATE_SHAPES)
def test_padded_even_ld_aligned(handle, M, N, K, ta, tb):
    A, B, want, bound = operands(M, N, K, ta, tb, 1000 + M + N + K)
    lda, ldb, offa, offb = gate_variant(M, N, K, ta, tb, "in")
    got = run_gemm(handle, M, N, K, ta, tb, A, B, lda, ldb, offa, offb)
    check(got, want, bound, "padded ld (%d, %d, %d) ta=%d tb=%d" % (M, N, K, ta, tb))


@pytest.mark.parametrize("M,N,ldb", [(256, 320, 322), (320, 256, 258)])
def test_padded_ld_eight_wave_tiles(handle, M, N, ldb):
    """12 entries of 256 x 320 x 32 (and the mirror): 192 tiles of 64x80 (80x64), the 8-wave pipeline tiles."""
    K, cnt, lda = 32, 12, 34
    rng = np.random.default_rng(M + 7 * N)
    As = [rng.standard_normal((M, K)) for _ in range(cnt)]
    Bs = [rng.standard_normal((K, N)) for _ in range(cnt)]
    eA = [embed(handle, a, lda, 2) for a in As]
    eB = [embed(handle, b, ldb, 2) for b in Bs]
    outs = [Guarded(handle, M, N) for _ in range(cnt)]
    handle.gemm_batched([o.view for o in outs], M, N, ALPHA, [e[0] for e in eA], lda, False, K, [e[0] for e in eB], ldb, False)
    for i in range(cnt):
        want, bound = reference(As[i], False, Bs[i], False)
        check(outs[i].result(), want, bound, "8-wave tiles (%d, %d, %d) entry %d" % (M, N, K, i))


@pytest.mark.parametrize("ta,tb", PAIRS)
@pytest.mark.parametrize("M,N,K", GATE_SHAPES)
def test_whole_tiles_off_the_gate(handle, M, N, K, ta, tb):
    """Odd lda, odd ldb, A 8 B off alignment: each meets the bound, and the four results on the same values (the
    pipeline's included) agree pairwise within twice the bound (different kernels: not bitwise)."""
    A, B, want, bound = operands(M, N, K, ta, tb, 1000 + M + N + K)
    res = {}
    for which in ("in", "lda", "ldb", "ptr"):
        lda, ldb, offa, offb = gate_variant(M, N, K, ta, tb, which)
        res[which] = run_gemm(handle, M, N, K, ta, tb, A, B, lda, ldb, offa, offb)
        check(res[which], want, bound, "off gate [%s] (%d, %d, %d) ta=%d tb=%d" % (which, M, N, K, ta, tb))
    names = list(res)
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            d = np.abs(res[names[i]].astype(LD) - res[names[j]].astype(LD))
            assert np.all(d <= 2 * bound), (names[i], names[j], float(np.max(d / bound)))


# ------------------------------------------------------------------ 3: ragged shapes, the general kernel
@pytest.mark.parametrize("ta,tb", PAIRS)
@pytest.mark.parametrize("M,N,K", [(33, 65, 47), (1, 37, 19), (37, 1, 19), (129, 131, 67), (13, 17, 1)])
def test_ragged_padded_ld(handle, M, N, K, ta, tb):
    A, B, want, bound = operands(M, N, K, ta, tb, 2000 + M + N + K)
    ra, rb = rowlens(M, N, K, ta, tb)
    got = run_gemm(handle, M, N, K, ta, tb, A, B, ra + 3, rb + 3, 1, 1)
    check(got, want, bound, "ragged (%d, %d, %d) ta=%d tb=%d" % (M, N, K, ta, tb))


# ------------------------------------------------------------------ 4: xrs_gemm_sym
def sym_pad(N):
    """(ld padding, offset): even / 16-B aligned for the whole-tile sizes (they stay on the pipeline), else odd."""
    return (2, 2) if N % 32 == 0 else (3, 1)


def check_sym(got, want, bound, label, exact_sym_product):
    assert np.array_equal(got, got.T), "%s: not exactly symmetric" % label
    if exact_sym_product:
        return check(got, want, bound, label)
    lo = np.tril(np.ones(got.shape, dtype=bool))
    want_m = np.where(lo, want, want.T)
    bound_m = np.where(lo, bound, bound.T)
    return check(got, want_m, bound_m, label)


@pytest.mark.parametrize("ta,tb", [(True, False), (False, True)])
@pytest.mark.parametrize("N,K", [(64, 256), (96, 128), (33, 17), (100, 300)])
def test_gemm_sym_padded_ld(handle, N, K, ta, tb):
    """X^T X (ta) and X X^T (tb) with A = B = X, one padded operand passed twice as the Gram callers do."""
    X = np.random.default_rng(3000 + N + K).standard_normal((K, N) if ta else (N, K))
    pad, off = sym_pad(N)
    ld = X.shape[1] + pad
    dX, keep = embed(handle, X, ld, off)
    out = Guarded(handle, N, N)
    handle.gemm_sym(out.view, N, ALPHA, dX, ld, ta, K, dX, ld, tb)
    want, bound = reference(X, ta, X, tb)
    check_sym(out.result(), want, bound, "sym (%d, %d) ta=%d tb=%d" % (N, K, ta, tb), True)


@pytest.mark.parametrize("ta", [True, False])
@pytest.mark.parametrize("N,K", [(33, 17), (100, 300)])
def test_gemm_sym_congruence_padded_ld(handle, N, K, ta):
    """X^T (G_s X) / (X G_s) X^T with G_s symmetric: A and B differ, the product is symmetric."""
    rng = np.random.default_rng(3500 + N + K)
    X = rng.standard_normal((K, N) if ta else (N, K))
    G = rng.standard_normal((K, K))
    Gs = G + G.T
    A, B = (X, Gs @ X) if ta else (X @ Gs, X)
    tb = not ta
    lda, ldb = A.shape[1] + 3, B.shape[1] + 3
    dA, keepA = embed(handle, A, lda, 1)
    dB, keepB = embed(handle, B, ldb, 1)
    out = Guarded(handle, N, N)
    handle.gemm_sym(out.view, N, ALPHA, dA, lda, ta, K, dB, ldb, tb)
    want, bound = reference(A, ta, B, tb)
    check_sym(out.result(), want, bound, "sym congruence (%d, %d) ta=%d" % (N, K, ta), False)


# ------------------------------------------------------------------ 5: xrs_gemm_batched
@pytest.mark.parametrize("ta,tb", PAIRS)
def test_batched_one_entry_misaligned(handle, ta, tb):
    """Only entry 1's A is 8 B off 16-B alignment: the whole batch has to leave the pipeline."""
    M = N = K = 64
    cnt = 3
    rng = np.random.default_rng(4000 + 2 * ta + tb)
    As = [rng.standard_normal(shape_of(M, K, ta)) for _ in range(cnt)]
    Bs = [rng.standard_normal(shape_of(N, K, not tb)) for _ in range(cnt)]
    ra, rb = rowlens(M, N, K, ta, tb)
    eA = [embed(handle, As[i], ra, 1 if i == 1 else 0) for i in range(cnt)]
    eB = [embed(handle, Bs[i], rb, 0) for i in range(cnt)]
    outs = [Guarded(handle, M, N) for _ in range(cnt)]
    handle.gemm_batched([o.view for o in outs], M, N, ALPHA, [e[0] for e in eA], ra, ta, K, [e[0] for e in eB], rb, tb)
    for i in range(cnt):
        want, bound = reference(As[i], ta, Bs[i], tb)
        check(outs[i].result(), want, bound, "batch of 3, entry %d ta=%d tb=%d" % (i, ta, tb))


@pytest.mark.parametrize("ta,tb", PAIRS)
def test_batched_across_launch_limit_padded_ld(handle, ta, tb):
    """33 entries (one launch holds 32) of 32 x 32 x 32 with lda = 34."""
    M = N = K = 32
    cnt, lda, ldb = 33, 34, 32
    rng = np.random.default_rng(4100 + 2 * ta + tb)
    As = rng.standard_normal((cnt, 32, 32))
    Bs = rng.standard_normal((cnt, 32, 32))
    eA = [embed(handle, As[i], lda, 2) for i in range(cnt)]
    eB = [embed(handle, Bs[i], ldb, 0) for i in range(cnt)]
    outs = [Guarded(handle, M, N) for _ in range(cnt)]
    handle.gemm_batched([o.view for o in outs], M, N, ALPHA, [e[0] for e in eA], lda, ta, K, [e[0] for e in eB], ldb, tb)
    for i in range(cnt):
        want, bound = reference(As[i], ta, Bs[i], tb)
        check(outs[i].result(), want, bound, "batch of 33, entry %d ta=%d tb=%d" % (i, ta, tb))


# ------------------------------------------------------------------ 6: the symmetric batch (export, sym = 1)
@pytest.mark.parametrize("N,K", [(64, 256), (40, 50)])
def test_symmetric_batch(handle, N, K):
    """Two Grams X_i X_i^T in one symmetric batch: exactly symmetric, inside the bound, and within twice the bound
    of the same product through xrs_gemm_sym."""
    cnt = 2
    rng = np.random.default_rng(5000 + N + K)
    Xs = [rng.standard_normal((N, K)) for _ in range(cnt)]
    pad, off = sym_pad(N)
    ld = K + pad
    eX = [embed(handle, x, ld, off) for x in Xs]
    dX = [e[0] for e in eX]
    outs = [Guarded(handle, N, N) for _ in range(cnt)]
    handle.gemm_forms([o.view for o in outs], N, N, ALPHA, dX, ld, False, K, dX, ld, True, sym=True)
    for i in range(cnt):
        want, bound = reference(Xs[i], False, Xs[i], True)
        got = outs[i].result()
        check_sym(got, want, bound, "symmetric batch (%d, %d) entry %d" % (N, K, i), True)
        single = Guarded(handle, N, N)
        handle.gemm_sym(single.view, N, ALPHA, dX[i], ld, False, K, dX[i], ld, True)
        d = np.abs(got.astype(LD) - single.result().astype(LD))
        assert np.all(d <= 2 * bound), (i, float(np.max(d / bound)))


# ------------------------------------------------------------------ 7: triangular skipping (export, tri = 1 / 2)
def tri_case(handle, cnt, M, N, K, tri, expect_skip):
    rng = np.random.default_rng(6000 + M + N + K + tri + cnt)
    As = [rng.standard_normal((M, K)) for _ in range(cnt)]
    Bs = [rng.standard_normal((K, N)) for _ in range(cnt)]
    if tri == 1:
        As = [np.tril(a) for a in As]      # A[m][k] = 0 for k > m (exact zeros)
    else:
        Bs = [np.tril(b) for b in Bs]      # B[k][n] = 0 for k < n
    pad, off = (2, 2) if (M % 32 == 0 and N % 32 == 0 and K % 32 == 0) else (3, 1)
    lda, ldb = K + pad, N + pad
    eA = [embed(handle, a, lda, off) for a in As]
    eB = [embed(handle, b, ldb, off) for b in Bs]
    dA, dB = [e[0] for e in eA], [e[0] for e in eB]
    res = {}
    flops = None
    for t in (tri, 0):
        outs = [Guarded(handle, M, N) for _ in range(cnt)]
        if t:
            handle.prof_begin(capi.KFAM_GEMM)
        handle.gemm_forms([o.view for o in outs], M, N, ALPHA, dA, lda, False, K, dB, ldb, False, tri=t)
        if t:
            flops = handle.prof_end()["flops"]
        res[t] = [o.result() for o in outs]
    label = "tri=%d count=%d (%d, %d, %d)" % (tri, cnt, M, N, K)
    for i in range(cnt):
        want, bound = reference(As[i], False, Bs[i], False)
        check(res[tri][i], want, bound, "%s entry %d" % (label, i))
        # skipped K-steps hold products with an exact zero only, and neither the tile variant nor the slice
        # partition depends on tri: the same bits
        assert np.array_equal(res[tri][i].view(np.uint64), res[0][i].view(np.uint64)), \
            "%s entry %d: differs from tri = 0" % (label, i)
    dense = cnt * 2.0 * M * N * K
    # the products that do not hold a structural zero: no correct kernel executes fewer
    if tri == 1:
        needed = cnt * 2.0 * N * sum(min(K, m + 1) for m in range(M))
    else:
        needed = cnt * 2.0 * M * sum(max(0, K - n) for n in range(N))
    print("%s: executed flops / dense = %.3f (needed %.3f)" % (label, flops / dense, needed / dense))
    assert needed <= flops <= dense, (needed, flops, dense)
    if expect_skip:
        assert flops < dense, (flops, dense)


@pytest.mark.parametrize("cnt,M,N,K,tri", [
    (1, 128, 128, 128, 1),
    (1, 256, 256, 256, 1),   # two K slices: tile row 0's second slice has no K-step and must still write zeros
    (1, 320, 128, 128, 2),
    (1, 256, 256, 256, 2),   # two K slices: the last tile column's first slice has no K-step
    (2, 128, 128, 128, 1),   # the bidiagonal SVD's batched form
    # 192 tiles of 80x64 / 64x80 (8 waves): tile rows end / tile columns begin off a K-step boundary, so the
    # rounding direction of the skipped range matters; B (128 x 320) has whole tile columns of zeros, whose
    # results are exact zeros from workgroups without a K-step
    (12, 320, 256, 128, 1),
    (12, 256, 320, 128, 2),
])
def test_triangular_skipping(handle, cnt, M, N, K, tri):
    tri_case(handle, cnt, M, N, K, tri, True)


def test_triangular_ragged_ignores_tri(handle):
    """A ragged shape runs the general kernel, which ignores tri: the bound and the same bits as tri = 0."""
    tri_case(handle, 1, 100, 70, 100, 1, False)


# ------------------------------------------------------------------ 8: argument checks
def test_argument_checks_fp64(handle):
    M, N, K = 8, 6, 4
    rng = np.random.default_rng(8)
    A, B = handle.array(rng.standard_normal((M, K))), handle.array(rng.standard_normal((K, N)))
    S = handle.array(rng.standard_normal((M, M)))   # square operand for the symmetric entry points
    C, C2 = handle.empty((M, N)), handle.empty((M, N))
    Cs = handle.empty((M, M))
    bad = [
        # lda too small, ldb too small, C aliasing A, C aliasing B
        lambda: handle.gemm(C, M, N, 1.0, A, K - 1, False, K, B, N, False),
        lambda: handle.gemm(C, M, N, 1.0, A, K, False, K, B, N - 1, False),
        lambda: handle.gemm(A, M, N, 1.0, A, K, False, K, B, N, False),
        lambda: handle.gemm(B, M, N, 1.0, A, K, False, K, B, N, False),
        lambda: handle.gemm_batched([C, C2], M, N, 1.0, [A, A], K - 1, False, K, [B, B], N, False),
        lambda: handle.gemm_batched([C, C2], M, N, 1.0, [A, A], K, False, K, [B, B], N - 1, False),
        lambda: handle.gemm_batched([C, A], M, N, 1.0, [A, A], K, False, K, [B, B], N, False),
        lambda: handle.gemm_batched([C, B], M, N, 1.0, [A, A], K, False, K, [B, B], N, False),
        lambda: handle.gemm_sym(Cs, M, 1.0, S, M - 1, True, M, S, M, False),
        lambda: handle.gemm_sym(Cs, M, 1.0, S, M, True, M, S, M - 1, False),
        lambda: handle.gemm_sym(S, M, 1.0, S, M, True, M, Cs, M, False),
        lambda: handle.gemm_sym(S, M, 1.0, Cs, M, True, M, S, M, False),
        lambda: handle.gemm_forms([C, C2], M, N, 1.0, [A, A], K - 1, False, K, [B, B], N, False),
        lambda: handle.gemm_forms([C, C2], M, N, 1.0, [A, A], K, False, K, [B, B], N - 1, False),
        lambda: handle.gemm_forms([C, A], M, N, 1.0, [A, A], K, False, K, [B, B], N, False),
        lambda: handle.gemm_forms([C, B], M, N, 1.0, [A, A], K, False, K, [B, B], N, False),
        lambda: handle.gemm_forms([A], M, N, 1.0, [A], K, False, K, [B], N, False),
        # the export's own rules: tri out of range, sym with M != N, sym and tri together
        lambda: handle.gemm_forms([C], M, N, 1.0, [A], K, False, K, [B], N, False, tri=3),
        lambda: handle.gemm_forms([C], M, N, 1.0, [A], K, False, K, [B], N, False, tri=-1),
        lambda: handle.gemm_forms([C], M, N, 1.0, [A], K, False, K, [B], N, False, sym=True),
        lambda: handle.gemm_forms([Cs], M, M, 1.0, [S], M, True, M, [S], M, False, sym=True, tri=1),
    ]
    for k, call in enumerate(bad):
        try:
            call()
        except capi.XrsError:
            continue
        pytest.fail("bad call %d was accepted" % k)
    # the handle still works, through the plain entry point and the export
    handle.gemm(C, M, N, ALPHA, A, K, False, K, B, N, False)
    handle.gemm_forms([C2], M, N, ALPHA, [A], K, False, K, [B], N, False)
    want, bound = reference(A.numpy(), False, B.numpy(), False)
    check(C.numpy(), want, bound, "after the rejected calls")
    assert np.array_equal(C2.numpy(), C.numpy())
