"""The UQ-ADF per-sample kernels (xerus_amd/csrc/uq.hip) through the C-ABI against NumPy (einsum / batched matmul).

Tolerances: the congruence is two chained fp64 products of inner lengths n and a (then a again), every sum in
one fixed order, so an entry is off by at most ~(n + 2a) eps times the product of the operand norms; with
a <= 256 and n <= 4 that is < 6e-14 of it in the worst case: 1e-13 of the sample's reference norm is the bound
used per sample.
"""
import ctypes as C

import numpy as np
import pytest

import uq_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (16, 16), (17, 16), (16, 33), (40, 7)]


def _inputs(N, a, n, b, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((a, n, b))
    P = uq_ref.hermite(rng.standard_normal(N), n)
    G = rng.standard_normal((N, a, a))
    L = (G.transpose(0, 2, 1) @ G) / a           # symmetric positive semi-definite, like a leftIs stack
    L = 0.5 * (L + L.transpose(0, 2, 1))         # exactly symmetric, as the kernel's own output is
    V = rng.standard_normal((N, a))
    return X, P, L, V


def _check_congruence(handle, N, a, n, b, with_l, seed=0):
    X, P, L, _ = _inputs(N, a, n, b, seed)
    M = np.einsum('jt,atb->jab', P, X)
    Mt = M.transpose(0, 2, 1)
    want = Mt @ L @ M if with_l else Mt @ M
    dX, dP = handle.array(X), handle.array(P)
    dL = handle.array(L) if with_l else None
    got = handle.uq_stack_congruence(dL, dX, dP).numpy()
    again = handle.uq_stack_congruence(dL, dX, dP).numpy()
    assert got.shape == (N, b, b)
    err = np.linalg.norm((got - want).reshape(N, -1), axis=1)
    scale = np.linalg.norm(want.reshape(N, -1), axis=1)
    print("congruence N=%d a=%d n=%d b=%d L=%s: max rel err %.3e" % (N, a, n, b, with_l, (err / scale).max()))
    assert np.all(err <= 1e-13 * scale)
    assert np.array_equal(got, got.transpose(0, 2, 1))      # exactly symmetric
    assert np.array_equal(got, again)                       # the same bits run to run


@pytest.mark.parametrize("with_l", [False, True])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("a,b", SHAPES)
def test_stack_congruence(handle, a, b, n, N, with_l):
    _check_congruence(handle, N, a, n, b, with_l, seed=a * 1000 + b * 10 + n)


@pytest.mark.parametrize("with_l", [False, True])
@pytest.mark.parametrize("a,b", [(112, 96), (256, 17), (130, 130)])
def test_stack_congruence_beyond_the_on_chip_tile(handle, a, b, with_l):
    """Shapes whose M_j and L_j M_j exceed what the tiled kernel keeps on chip, or with one rank below a tile
    and M_j beyond one sample slot: the column-panel path. 112 x 96 without L still fits the tiled kernel, with
    more than 64 KiB of LDS."""
    _check_congruence(handle, 3, a, 2, b, with_l, seed=a + b)


@pytest.mark.parametrize("with_l", [False, True])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("a", sorted({s[0] for s in SHAPES}))
def test_quadform(handle, a, N, with_l):
    _check_quadform(handle, a, N, with_l)


@pytest.mark.parametrize("with_l", [False, True])
def test_quadform_largest_rank(handle, with_l):
    _check_quadform(handle, 256, 5, with_l)


def _check_quadform(handle, a, N, with_l):
    _, _, L, V = _inputs(N, a, 1, 1, a + N)
    terms = np.einsum('ja,jab,jb->j', V, L, V) if with_l else np.einsum('ja,ja->j', V, V)
    dV = handle.array(V)
    dL = handle.array(L) if with_l else None
    got = handle.uq_quadform(dL, dV)
    # |error| <= (a + log2 N a) eps sum_j |v_j|^T |L_j| |v_j| <= 1e-13 of that sum for a <= 256
    bound = np.einsum('ja,jab,jb->', np.abs(V), np.abs(L), np.abs(V)) if with_l else terms.sum()
    print("quadform N=%d a=%d L=%s: err / bound %.3e" % (N, a, with_l, abs(got - terms.sum()) / bound))
    assert abs(got - terms.sum()) <= 1e-13 * bound
    assert handle.uq_quadform(dL, dV) == got


@pytest.mark.parametrize("n", [1, 2, 7])
def test_basis(handle, n):
    v = np.concatenate([np.linspace(-6.0, 6.0, 255), [0.0, 1e-300]])
    got = handle.uq_basis(handle.array(v), n).numpy()
    want = uq_ref.hermite(v, n)
    assert got.shape == (v.size, n)
    assert np.all(np.linalg.norm(got - want, axis=1) <= 1e-14 * np.linalg.norm(want, axis=1))
    # entry by entry: the same recurrence in the same order, up to a fused multiply-add (one rounding less per
    # step). Relative to the largest term of the recurrence at that v, as cancellation near a root of He_i has
    # no relative bound.
    scale = np.maximum.accumulate(np.abs(want), axis=1)
    assert np.all(np.abs(got - want) <= 1e-14 * scale)


def test_refused_shapes(handle):
    lib, h = handle.lib, handle.h
    buf = handle.zeros((257 * 257,))
    p = C.c_void_p(buf.ptr)
    r = C.c_double()
    assert lib.xrs_uq_stack_congruence(h, p, None, p, p, 1, 257, 1, 1) < 0
    assert lib.xrs_uq_stack_congruence(h, p, None, p, p, 1, 1, 1, 257) < 0
    assert lib.xrs_uq_stack_congruence(h, p, None, p, p, 1, 0, 1, 1) < 0
    assert lib.xrs_uq_stack_congruence(h, p, None, p, p, 1, 1, 0, 1) < 0
    assert lib.xrs_uq_stack_congruence(h, p, p, p, p, 1, 2, 1, 2) < 0       # Lout aliases Lprev
    assert lib.xrs_uq_stack_congruence(h, None, None, p, p, 1, 2, 1, 2) < 0
    assert lib.xrs_uq_quadform(h, C.byref(r), None, p, 1, 257) < 0
    assert lib.xrs_uq_quadform(h, C.byref(r), None, p, 1, 0) < 0
    assert lib.xrs_uq_quadform(h, None, None, p, 1, 1) < 0
    assert lib.xrs_uq_basis(h, None, p, 3, 2) < 0
    assert lib.xrs_last_error()
