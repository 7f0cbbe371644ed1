"""Ports of the reference's four active tests of the Riemannian layer (src/unitTests/retractions.cxx:27-258):
retractions at zero and at a 1e-3 change, tangent-vector orthogonality, tangent-vector creation and the
projective vector transport.

Inputs are drawn from numpy.random.default_rng(seed) and set through set_component. Each inequality uses the
reference's bound; where the NumPy restatement (tests/riemannian_ref.py) evaluated on the same inputs -- with
the base cores read back from the GPU, so in the same gauge -- does not stay ten times inside that bound, the
bound is ten times the restatement's own value (the factor covers a different summation order): _bound().
The figures that need this track cond(UU_k) (2e2 .. 6.7e4 over 20 seeds of the [2,3,5,4,3,2,4,1,2] shape):
P^2 = P ranges from 3e-16 to 4.5e-11 and the transported components up to 5e-12 there, so the literal 1e-14 and
1e-13 are not safe for an arbitrary seed. Bounds used, reference line in brackets:
    zero-direction components 1e-14 [:37]; retraction at zero 1e-8 [:43-69]; change components > 1e-10 [:79];
    gauge ||V_k U_k^T|| 1e-15 ||V_k|| [:81]; angle 100 EPS^2, EPS 1e-4 < |change| < EPS [:94-146];
    P b = b 1e-13, |<delta - P delta, b>| 1e-9, <delta, b> = <P delta, b> within 2e-10 [:171-177];
    norms 1e-14, scalar product 1e-10, a - a 1e-14, P^2 = P 1e-14, base 10 X 1e-14 [:192-226];
    transport to the same base 1e-13, 1 - |angle| max(eps^2, 1e-15), norm growth 1e-13 [:244-256].
"""
import numpy as np
import pytest

import riemannian_ref as rr

pytestmark = pytest.mark.gpu

REF_DIMS, REF_RANKS = [2, 3, 5, 4, 3, 2, 4, 1, 2], [2, 2, 4, 1, 3, 4, 2, 2]


def _bound(reference_bound, restated_value):
    return reference_bound if 10.0 * restated_value <= reference_bound else 10.0 * restated_value


def _approx_equal_gap(a, b):
    """misc::approx_equal(a, b, eps) holds iff |a - b| <= eps * this (misc/math.h:71-73)."""
    return 0.5 * (abs(a) + abs(b))


def _tensor(xe, arr):
    return xe.Tensor.from_ndarray(np.require(np.asarray(arr, dtype=np.float64), requirements="C"))


def _random_cores(rng, dims, ranks):
    r = [1] + list(ranks) + [1]
    return [rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))]


def _tt(xe, cores, move=True):
    t = xe.TTTensor([c.shape[1] for c in cores])
    for k, c in enumerate(cores):
        t.set_component(k, _tensor(xe, c))
    if move:
        t.move_core(0)
    return t


def _cores(tt):
    return [tt.get_component(k).to_ndarray() for k in range(tt.degree())]


def _oracle(ref, tt):
    o = ref.TT(_cores(tt))
    o.canonicalized, o.core_position = tt.canonicalized, tt.corePosition
    return o


def _full(xe, tt):
    return xe.Tensor(tt).to_ndarray()


def _norms(components):
    return [float(np.linalg.norm(c)) for c in components]


def _gpu_components(tv):
    return [c.to_ndarray() for c in tv.components]


# ------------------------------------------------------------------------------------------ retractions
EPS = 1e-3
RETRACTIONS = [   # (name, takes a tangent vector)
    ("ALSRetractionI", True), ("ALSRetractionII", False), ("SubmanifoldRetractionI", True), ("SubmanifoldRetractionII", False),
    ("HOSVDRetraction(2)", True), ("HOSVDRetraction(2)", False), ("HOSVDRetractionI", True), ("HOSVDRetractionII", False),
]


def _retraction(xe, name):
    return xe.HOSVDRetraction(2) if name == "HOSVDRetraction(2)" else getattr(xe, name)


@pytest.fixture(scope="module")
def retraction_case(xe, ref):
    rng = np.random.default_rng(5)
    dims, ranks = [4] * 8, [2] * 7
    X = _tt(xe, _random_cores(rng, dims, ranks))
    zero = _tt(xe, _random_cores(rng, dims, ranks))
    zero *= 1e-16
    change = _tt(xe, _random_cores(rng, dims, ranks))
    change *= EPS / change.frob_norm()
    tangent_zero = xe.TTTangentVector(X, zero)
    tangent_change = xe.TTTangentVector(X, change)
    riemannian = tangent_change.to_tt()
    riemannian /= riemannian.frob_norm()
    base = _cores(tangent_change.baseL)
    return dict(X=X, zero=zero, change=change, tangent_zero=tangent_zero, tangent_change=tangent_change, riemannian=riemannian,
                base=base, want_zero=rr.project(base, _cores(zero)), want_change=rr.project(base, _cores(change)))


def test_projection_of_zero_and_of_a_small_change(xe, retraction_case):
    c = retraction_case
    for got, want in zip(_norms(_gpu_components(c["tangent_zero"])), _norms(c["want_zero"].components)):
        assert got < _bound(1e-14, want)                                                   # :37
    comps = _gpu_components(c["tangent_change"])
    for k, V in enumerate(comps):
        assert np.linalg.norm(V) > 1e-10                                                   # :79
        if k != 0:   # :81, relative to ||V_k||
            got = np.linalg.norm(np.einsum('arj,brj->ab', V, c["base"][k])) / np.linalg.norm(V)
            Vw = c["want_change"].components[k]
            want = np.linalg.norm(np.einsum('arj,brj->ab', Vw, c["base"][k])) / np.linalg.norm(Vw)
            print(f"gauge {k}: {got:.2e} (restatement {want:.2e})")
            assert got < _bound(1e-15, want)


@pytest.mark.parametrize("name,tangent", RETRACTIONS)
def test_retraction_at_zero(xe, retraction_case, name, tangent):
    c = retraction_case
    Y = xe.TTTensor(c["X"])
    _retraction(xe, name)(Y, c["tangent_zero"] if tangent else c["zero"])
    assert Y.ranks() == c["X"].ranks()
    assert xe.frob_norm(c["X"] - Y) < 1e-8                                                 # :43-69


@pytest.mark.parametrize("name,tangent", RETRACTIONS)
def test_retraction_at_small_change(xe, retraction_case, name, tangent):
    c = retraction_case
    Y = xe.TTTensor(c["X"])
    _retraction(xe, name)(Y, c["tangent_change"] if tangent else c["change"])
    actual = Y - c["X"]
    fnorm = xe.frob_norm(actual)
    angle = 1 - xe.dot(c["riemannian"], actual) / fnorm
    print(f"{name}: |change| {fnorm:.3e}, angle {angle:.3e}")
    assert angle < 100 * EPS * EPS                                                         # :94-146
    assert EPS * 1e-4 < fnorm < EPS


# ------------------------------------------------------------------------------------------ orthogonality
def test_tangent_vector_orthogonality(xe, ref):
    """Every TT with one component of X replaced by a unit tensor lies in the tangent space: P b = b, and
    delta - P delta is orthogonal to it (:151-180)."""
    rng = np.random.default_rng(5)
    X = _tt(xe, _random_cores(rng, REF_DIMS, REF_RANKS))
    dcores = _random_cores(rng, REF_DIMS, REF_RANKS)
    delta = _tt(xe, dcores)
    tv = xe.TTTangentVector(X, delta)
    base = _cores(tv.baseL)
    dfull = ref.TT(dcores).full()
    pfull = _full(xe, tv.to_tt())
    want_pfull = rr.full(rr.project(base, dcores))
    worst = [0.0, 0.0, 0.0]
    for n, U in enumerate(base):
        for i in range(U.size):
            bcores = [c.copy() for c in base]
            e = np.zeros(U.size)
            e[i] = 1.0
            bcores[n] = e.reshape(U.shape)
            bfull = ref.TT(bcores).full()
            b = xe.TTTensor(X)
            b.set_component(n, _tensor(xe, bcores[n]))
            b.move_core(0)
            pb = _full(xe, xe.TTTangentVector(X, b).to_tt())
            want_pb = rr.full(rr.project(base, bcores))
            nb = np.linalg.norm(bfull)
            got, want = np.linalg.norm(bfull - pb) / nb, np.linalg.norm(bfull - want_pb) / nb
            assert got < _bound(1e-13, want), (n, i)                                       # :171
            db, pdb, want_pdb = float(np.vdot(dfull, bfull)), float(np.vdot(pfull, bfull)), float(np.vdot(want_pfull, bfull))
            assert abs(db - pdb) < _bound(1e-9, abs(db - want_pdb)), (n, i)                # :175
            gap = 2e-10 * _approx_equal_gap(db, pdb)
            assert abs(db - pdb) <= _bound(gap, abs(db - want_pdb)), (n, i)                # :177
            worst = [max(worst[0], got), max(worst[1], abs(db - pdb)), max(worst[2], abs(db - pdb) / max(gap, 1e-300))]
    print("worst |b - Pb|/|b| %.2e, |<delta - P delta, b>| %.2e, that over the approx_equal gap %.2e" % tuple(worst))


# ------------------------------------------------------------------------------------------ creation
@pytest.mark.parametrize("seed", [5, 1])
def test_tangent_vector_creation(xe, ref, seed):
    rng = np.random.default_rng(seed)
    X = _tt(xe, _random_cores(rng, REF_DIMS, REF_RANKS))
    ccores, c2cores = _random_cores(rng, REF_DIMS, REF_RANKS), _random_cores(rng, REF_DIMS, REF_RANKS)
    change, change2 = _tt(xe, ccores), _tt(xe, c2cores)
    t1 = xe.TTTangentVector(X, change)
    base = _cores(t1.baseL)
    w1, w2 = rr.project(base, ccores), rr.project(base, c2cores)
    w1tt = rr.to_tt(w1)

    # projection should decrease norm (:192)
    emb = t1.to_tt().frob_norm()
    assert change.frob_norm() > emb
    # norm in the tangent space against the embedding norm (:195-202)
    want_gap = abs(rr.tt_norm(w1tt) - rr.frob_norm(w1))
    for tangent_norm in (np.sqrt(t1.scalar_product(t1)), t1.frob_norm()):
        assert abs(emb - tangent_norm) <= _bound(1e-14 * _approx_equal_gap(emb, tangent_norm), want_gap)
    # scalar product of two vectors (:204-210)
    t2 = xe.TTTangentVector(X, change2)
    sp_t, sp_e = t1.scalar_product(t2), xe.dot(t1.to_tt(), t2.to_tt())
    want_sp_gap = abs(rr.scalar_product(w1, w2) - float(np.vdot(rr.full(w1), rr.full(w2))))
    assert abs(sp_t - sp_e) <= _bound(1e-10 * _approx_equal_gap(sp_t, sp_e), want_sp_gap)
    # copy, += and * (:213-217)
    t2 = xe.TTTangentVector(t1)
    t2 += t1 * (-1)
    for c in t2.components:
        assert xe.frob_norm(c) < 1e-14
    # projection P P = P (:220-222); tracks cond(UU)
    t2 = xe.TTTangentVector(X, t1.to_tt())
    wpp = rr.project(base, w1tt.cores)
    n1, nw = t1.frob_norm(), rr.frob_norm(w1)
    pp1, want_pp1 = (t2.frob_norm() - n1) / n1, abs(rr.frob_norm(wpp) - nw) / nw
    pp2 = xe.frob_norm(t1.to_tt() - t2.to_tt()) / n1
    want_pp2 = np.linalg.norm(rr.full(w1) - rr.full(wpp)) / nw
    print(f"seed {seed}: PP {pp1:.2e} (restatement {want_pp1:.2e}), PP2 {pp2:.2e} (restatement {want_pp2:.2e})")
    assert pp1 < _bound(1e-14, want_pp1)
    assert pp2 < _bound(1e-14, want_pp2)
    # tangent space of 10 X equals the tangent space of X (:225-226)
    X10 = 10 * X
    t10 = xe.TTTangentVector(X10, change)
    w10 = rr.project(_cores(t10.baseL), ccores)
    x10 = xe.frob_norm(t1.to_tt() - t10.to_tt()) / n1
    want_x10 = np.linalg.norm(rr.full(w1) - rr.full(w10)) / nw
    print(f"seed {seed}: 10X {x10:.2e} (restatement {want_x10:.2e})")
    assert x10 < _bound(1e-14, want_x10)


# ------------------------------------------------------------------------------------------ vector transport
def test_vector_transport(xe, ref):
    rng = np.random.default_rng(5)
    dims, ranks = [4] * 8, [2] * 7
    X = _tt(xe, _random_cores(rng, dims, ranks))
    ccores = _random_cores(rng, dims, ranks)
    t1 = xe.TTTangentVector(X, _tt(xe, ccores))
    base = _cores(t1.baseL)
    w1 = rr.project(base, ccores)
    oX = _oracle(ref, X)

    # vector transport from X to X should not change the vector at all (:240-245)
    t2 = xe.TTTangentVector(t1)
    xe.ProjectiveVectorTransport(X, t2)
    t2 -= t1
    wsame = rr.projective_transport(oX, w1)
    for got, a, b in zip(_norms(_gpu_components(t2)), wsame.components, w1.components):
        assert got < _bound(1e-13, float(np.linalg.norm(a - b)))

    norm_old, want_old = t1.frob_norm(), rr.frob_norm(w1)
    t1tt = t1.to_tt()
    w1full = rr.full(w1)
    for eps in [1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4]:                                # :248-257
        newX = xe.TTTensor(X)
        xe.SubmanifoldRetractionI(newX, t1 * eps)
        assert newX.canonicalized and newX.corePosition == 0
        t2 = xe.TTTangentVector(t1)
        xe.ProjectiveVectorTransport(newX, t2)
        norm_new = t2.frob_norm()
        angle = xe.dot(t1tt, t2.to_tt()) / norm_old / norm_new
        wnew = rr.projective_transport(_oracle(ref, newX), w1)
        want_new = rr.frob_norm(wnew)
        want_angle = float(np.vdot(w1full, rr.full(wnew))) / want_old / want_new
        print(f"eps {eps:.0e}: 1-|angle| {1 - abs(angle):.2e} (restatement {1 - abs(want_angle):.2e}), "
              f"norm growth {norm_new - norm_old:.2e} (restatement {want_new - want_old:.2e})")
        assert 1 - abs(angle) < _bound(max(eps * eps, 1e-15), abs(1 - abs(want_angle)))
        assert norm_new - norm_old <= _bound(1e-13, max(0.0, want_new - want_old))
