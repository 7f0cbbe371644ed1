"""TTTangentVector on the GPU (tangent.hip through the host API) against the NumPy restatement
(tests/riemannian_ref.py, retractions.cpp:82-260).

The components depend on the gauge of the base, so the restatement gets the base cores read back from the
GPU object (as test_als_gpu.py does for ALS). Bar: 1e-9 relative, the project's bar for ALS. The largest
cond(UU_k) of the full-rank cases is 10, 1.4e4, 2e2 and 6.7e4, so cond * 2^-52 < 2e-11 leaves the restatement
itself well inside the bar. A component that vanishes in exact arithmetic (a square core) has no scale of its
own: component errors are measured against the largest component norm of the vector.
"""
import numpy as np
import pytest

import riemannian_ref as rr

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _random_cores(rng, dims, ranks):
    r = [1] + list(ranks) + [1]
    return [rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))]


def _tt(xe, cores):
    t = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        t.set_component(k, _tensor(xe, c))
    return t


def _cores(tt):
    return [tt.get_component(k).to_ndarray() for k in range(tt.degree())]


def _full(xe, tt):
    return xe.Tensor(tt).to_ndarray()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _check_against_restatement(xe, ref, X, Zcores, Z2cores):
    Z = _tt(xe, Zcores)
    tv = xe.TTTangentVector(X, Z)
    base = _cores(tv.baseL)
    want = rr.project(base, Zcores)
    got = [c.to_ndarray() for c in tv.components]
    scale = max(np.linalg.norm(c) for c in want.components)
    assert len(got) == len(base)
    for k in range(len(base)):
        assert got[k].shape == base[k].shape
        err = np.linalg.norm(got[k] - want.components[k]) / scale
        print(f"component {k}: rel err {err:.2e}")
        assert err <= TOL
    xfull = ref.TT(base).full()
    pfull = rr.full(want)
    tt = tv.to_tt()
    assert tt.canonicalized and tt.corePosition == 0
    assert _rel(_full(xe, tt), pfull) <= TOL
    assert _rel(_full(xe, tv.added_to_base()), xfull + pfull) <= TOL
    # scalar products: with itself, and with a second vector over the same base
    tv2 = xe.TTTangentVector(X, _tt(xe, Z2cores))
    want2 = rr.project(base, Z2cores)
    n1, n2 = rr.frob_norm(want), rr.frob_norm(want2)
    assert abs(tv.scalar_product(tv2) - rr.scalar_product(want, want2)) <= TOL * n1 * n2
    assert abs(tv.scalar_product(tv) - n1 * n1) <= TOL * n1 * n1
    assert tv.frob_norm() == pytest.approx(n1, rel=TOL)
    return tv, tv2


CASES = [
    # modes, base ranks, direction ranks, seed
    ([4, 5, 3, 4], [2, 3, 2], [3, 4, 3], 5),                                        # direction ranks above the base's
    ([6, 6, 6, 6], [6, 17, 6], [5, 9, 5], 5),                                       # past one MFMA tile, odd: scalar block path
    ([2, 3, 5, 4, 3, 2, 4, 1, 2], [2, 2, 4, 1, 3, 4, 2, 2], [2, 2, 4, 1, 3, 4, 2, 2], 5),   # the reference's own shape
    ([2, 3, 5, 4, 3, 2, 4, 1, 2], [2, 2, 4, 1, 3, 4, 2, 2], [2, 2, 4, 1, 3, 4, 2, 2], 1),
    ([2, 3], [2], [1], 5),                                                          # d = 2
    ([5], [], [], 5),                                                               # d = 1
]


@pytest.mark.parametrize("dims,ranks,zranks,seed", CASES)
def test_projection_matches_restatement(xe, ref, dims, ranks, zranks, seed):
    rng = np.random.default_rng(seed)
    X = _tt(xe, _random_cores(rng, dims, ranks))
    X.move_core(0)
    assert X.ranks() == ranks
    tv, tv2 = _check_against_restatement(xe, ref, X, _random_cores(rng, dims, zranks), _random_cores(rng, dims, zranks))
    assert tv.fallbackEdges == 0 and tv2.fallbackEdges == 0


def test_rank_deficient_base_takes_the_pseudo_inverse(xe, ref):
    """A rank-2 TT zero-padded to rank 3 and canonicalised with keepRank: every left Gram UU_k is singular, the
    Cholesky certificate fails and the edges go through the SVD pseudo-inverse, as the restatement's
    pinv(rcond = EPSILON) does."""
    rng = np.random.default_rng(5)
    dims = [4, 4, 4, 4]
    cores = []
    for k, c in enumerate(_random_cores(rng, dims, [2, 2, 2])):
        p = np.zeros((1 if k == 0 else 3, 4, 1 if k == 3 else 3))
        p[:c.shape[0], :, :c.shape[2]] = c
        cores.append(p)
    X = _tt(xe, cores)
    X.move_core(0, True)
    assert X.ranks() == [3, 3, 3]
    tv, tv2 = _check_against_restatement(xe, ref, X, _random_cores(rng, dims, [3, 3, 3]), _random_cores(rng, dims, [2, 4, 2]))
    assert tv.fallbackEdges >= 1 and tv2.fallbackEdges >= 1


def test_arithmetic_and_set_base(xe, ref):
    """+=, -=, *=, * on the components; the cached Grams are recomputed after set_base."""
    rng = np.random.default_rng(2)
    dims, ranks = [3, 4, 3], [2, 3]
    X = _tt(xe, _random_cores(rng, dims, ranks))
    X.move_core(0)
    a = xe.TTTangentVector(X, _tt(xe, _random_cores(rng, dims, ranks)))
    b = xe.TTTangentVector(X, _tt(xe, _random_cores(rng, dims, ranks)))
    ca, cb = [c.to_ndarray() for c in a.components], [c.to_ndarray() for c in b.components]
    s = xe.TTTangentVector(a)
    s += b * 0.5
    s -= 2.0 * a
    s *= 3.0
    for k in range(3):
        assert _rel(s.components[k].to_ndarray(), 3.0 * (0.5 * cb[k] - ca[k])) <= 1e-13
    base = _cores(a.baseL)
    want = rr.scalar_product(rr.Tangent(base, ca), rr.Tangent(base, cb))
    assert a.scalar_product(b) == pytest.approx(want, rel=TOL)
    a.set_base(X)   # drops the Grams: the next product recomputes them from baseL
    assert a.scalar_product(b) == pytest.approx(want, rel=TOL)


@pytest.mark.parametrize("ra,rb", [(1, 1), (3, 5), (16, 17), (5, 4)])
@pytest.mark.parametrize("add_base", [False, True])
def test_block_kernel_bit_exact(handle, ra, rb, add_base):
    """xrs_tt_tangent_to_tt alone: every core equals the NumPy block assembly bit for bit (copies, zeros and one
    fp64 addition per entry of the first core). (16, 17): the first core takes the 16-byte path, the interior
    one (odd r[k+1]) the 8-byte path; (5, 4): the reverse."""
    rng = np.random.default_rng(100 * ra + rb)
    n, r = [3, 4, 2], [1, ra, rb, 1]
    U = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(3)]
    V = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(3)]
    out = handle.tangent_to_tt(n, r, [handle.array(c) for c in U], [handle.array(c) for c in V], add_base)
    want = rr.block_cores(U, V, add_base)
    for k in range(3):
        assert out[k].shape == want[k].shape
        assert np.array_equal(out[k].numpy(), want[k])
