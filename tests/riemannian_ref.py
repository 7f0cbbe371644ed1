"""NumPy restatement of the reference's Riemannian TT algorithms (helper module, not collected).

    retractions.cpp:30-288      HOSVD / ALS / submanifold retractions, TTTangentVector, ProjectiveVectorTransport
    steepestDescent.cpp:37-176  line_search, SteepestDescentVariant::solve
    cg.cpp:38-124               GeometricCGVariant::solve

It builds on oracle.xerus_ref for the TT operations of the reference (move_core, round, ALS, sums, operator
application). TT cores are (r_k, n_k, r_{k+1}) arrays; a tangent vector is a Tangent(base cores, components).
Everything here is gauge dependent exactly where the reference is: the components belong to the base cores
given, so a test hands over the base cores of the object under test.
"""
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from oracle import xerus_ref as ref

EPSILON = ref.EPSILON


def pinv(G: np.ndarray) -> np.ndarray:
    """pseudo_inverse(G, 1) (tensor.cpp:1568-1574): singular values <= EPSILON * sigma_max dropped."""
    return np.linalg.pinv(G, rcond=EPSILON)


@dataclass
class Tangent:
    base: List[np.ndarray]          # baseL: right-orthogonal, core at 0
    components: List[np.ndarray]

    def copy(self) -> "Tangent":
        return Tangent([c.copy() for c in self.base], [c.copy() for c in self.components])

    def scaled(self, alpha: float) -> "Tangent":
        return Tangent(self.base, [alpha * c for c in self.components])


def left_grams(U: Sequence[np.ndarray]) -> List[np.ndarray]:
    """leftStackUU (retractions.cpp:99): UU[k+1](j1,j2) = UU[k](i1,i2) U_k(i1,r,j1) U_k(i2,r,j2), UU[0] = 1."""
    out = [np.ones((1, 1))]
    for Uk in U[:-1]:
        out.append(np.einsum('ab,arc,brd->cd', out[-1], Uk, Uk))
    return out


def project(U: Sequence[np.ndarray], Z: Sequence[np.ndarray]) -> Tangent:
    """TTTangentVector(base, direction) (retractions.cpp:82-130); U must be right-orthogonal with the core at 0."""
    d = len(U)
    UV, UU = [np.ones((1, 1))], [np.ones((1, 1))]
    for k in range(d - 1):
        UV.append(np.einsum('ab,arc,brd->cd', UV[-1], U[k], Z[k]))      # :97
        UU.append(np.einsum('ab,arc,brd->cd', UU[-1], U[k], U[k]))      # :99
    right = np.ones((1, 1))
    comps: List[Optional[np.ndarray]] = [None] * d
    for k in range(d - 1, -1, -1):
        V = np.einsum('as,sb,brc,jc->arj', pinv(UU[k]), UV[k], Z[k], right)   # :110-111
        if k != 0:
            UTV = np.einsum('arj,brj->ab', V, U[k])                     # :116
            V = V - np.einsum('as,srj->arj', UTV, U[k])                 # :117
            right = np.einsum('jra,krb,ab->jk', U[k], Z[k], right)      # :121
        comps[k] = V
    return Tangent([np.array(c, dtype=np.float64) for c in U], comps)   # type: ignore[arg-type]


def scalar_product(a: Tangent, b: Tangent) -> float:
    """TTTangentVector::scalar_product (retractions.cpp:167-179), over a's base."""
    G = left_grams(a.base)
    return float(sum(np.einsum('ab,arj,brj->', G[k], a.components[k], b.components[k]) for k in range(len(a.base))))


def frob_norm(a: Tangent) -> float:
    return float(np.sqrt(scalar_product(a, a)))


def block_cores(U: Sequence[np.ndarray], V: Sequence[np.ndarray], add_base: bool) -> List[np.ndarray]:
    """The rank-2r cores of operator TTTensor() / added_to_base() before move_core(0) (retractions.cpp:186-260)."""
    d = len(U)
    if d == 1:
        return [V[0] + U[0] if add_base else V[0].copy()]
    out = []
    for k in range(d):
        a, n, b = U[k].shape
        if k == 0:
            C = np.zeros((1, n, 2 * b))
            C[:, :, :b] = U[0]
            C[:, :, b:] = U[0] + V[0] if add_base else V[0]
        elif k == d - 1:
            C = np.zeros((2 * a, n, 1))
            C[:a] = V[k]
            C[a:] = U[k]
        else:
            C = np.zeros((2 * a, n, 2 * b))
            C[:a, :, :b] = U[k]
            C[:a, :, b:] = V[k]
            C[a:, :, b:] = U[k]
        out.append(C)
    return out


def to_tt(t: Tangent, add_base: bool = False) -> ref.TT:
    tt = ref.TT(block_cores(t.base, t.components, add_base))
    if len(t.base) > 1:
        tt.move_core(0)
    else:
        tt.canonicalized, tt.core_position = True, 0
    return tt


def full(t: Tangent, add_base: bool = False) -> np.ndarray:
    """Dense tensor of the tangent vector: sum_k U_0 .. V_k .. U_{d-1} (the commented form of :225-233)."""
    d = len(t.base)
    res = ref.TT(list(t.base)).full() if add_base else 0.0
    for k in range(d):
        cores = list(t.base)
        cores[k] = t.components[k]
        res = res + ref.TT(cores).full()
    return res


# ------------------------------------------------------------------------------------------------ TT helpers
def tt_scaled(x: ref.TT, alpha: float) -> ref.TT:
    y = x.copy()
    k = y.core_position if y.canonicalized else 0
    y.cores[k] = alpha * y.cores[k]
    return y


def tt_sub(x: ref.TT, y: ref.TT) -> ref.TT:
    return ref.tt_add(x, tt_scaled(ref.TT([c.copy() for c in y.cores]), -1.0))


def tt_norm(x: ref.TT) -> float:
    """frob_norm of a canonicalised copy (the reference's b - x is canonical: operator+= moves the core back,
    ttNetwork.cpp:841-843), so a small residual is not lost to the cancellation in <x, x>."""
    y = x.copy()
    y.move_core(0)
    return float(np.linalg.norm(y.cores[0]))


def assign(x: ref.TT, y: ref.TT):
    x.cores = [c.copy() for c in y.cores]
    x.canonicalized, x.core_position = y.canonicalized, y.core_position


# ------------------------------------------------------------------------------------------------ retractions
def hosvd_retraction(ranks) -> Callable:
    """HOSVDRetraction(rank) (retractions.cpp:30-48), for a TT change or a Tangent."""
    def apply(x: ref.TT, change):
        y = to_tt(change, add_base=True) if isinstance(change, Tangent) else ref.tt_add(x, change)
        y.round(ranks)
        assign(x, y)
    return apply


def hosvd_retraction_keep(x: ref.TT, change):
    """HOSVDRetractionI / II (retractions.cpp:50-60): round back to the ranks of x."""
    hosvd_retraction(list(x.ranks))(x, change)


def als_retraction(x: ref.TT, change):
    """ALSRetractionI / II (retractions.cpp:62-74): ALSVariant(1, 2, lapack_solver, false)(x, x + change)."""
    target = to_tt(change, add_base=True) if isinstance(change, Tangent) else ref.tt_add(x, change)
    ref.als(None, x, target, spd=False, num_half_sweeps=2)


def submanifold_retraction(x: ref.TT, change):
    """SubmanifoldRetractionI / II (retractions.cpp:264-277)."""
    w = change if isinstance(change, Tangent) else project(x.cores, change.cores)
    x.cores = [x.cores[k] + w.components[k] for k in range(x.order)]
    x.canonicalized = x.order == 1
    x.move_core(0, keep_rank=True)


def projective_transport(new_base: ref.TT, t: Tangent) -> Tangent:
    """ProjectiveVectorTransport (retractions.cpp:283-287)."""
    assert new_base.canonicalized and new_base.core_position == 0
    return project(new_base.cores, to_tt(t).cores)


# ------------------------------------------------------------------------------------------------ solvers
def _residual(A, x: ref.TT, b: ref.TT) -> ref.TT:
    if A is None:
        return tt_sub(b, x)
    return tt_sub(b, ref.TT(ref.op_apply_cores(A, x.cores)))


def steepest_descent(A, x: ref.TT, b: ref.TT, num_steps: int, eps: float, retraction: Callable, spd: bool = False) -> List[float]:
    """SteepestDescentVariant::solve (steepestDescent.cpp:83-176); x is updated in place. Returns the residual
    before the first step followed by the residual after every step."""
    residual = _residual(A, x, b)
    curr, last = tt_norm(residual), 1e100
    hist = [curr]
    alpha, steps = 1.0, 0
    while (num_steps == 0 or steps < num_steps) and curr > eps and abs(last - curr) > eps and abs(1 - curr / last) > eps:
        steps += 1
        if A is not None and not spd:
            y = ref.TT(ref.op_apply_cores(A, residual.cores, transpose=True))   # y = A^T (b - A x)
        else:
            y = residual
        old = x.copy()
        alpha *= 2
        retraction(x, tt_scaled(y, alpha))
        last = curr
        residual = _residual(A, x, b)
        curr = tt_norm(residual)
        while alpha > 1e-30 and last < curr:   # armijo backtracking (:164-170)
            alpha /= 2
            assign(x, old)
            retraction(x, tt_scaled(y, alpha))
            residual = _residual(A, x, b)
            curr = tt_norm(residual)
        hist.append(curr)
    return hist


def line_search(x: ref.TT, alpha: float, direction: Tangent, derivative: float, residual: float, retraction: Callable,
                calculate_residual: Callable[[], float], change_in_alpha: float):
    """line_search (steepestDescent.cpp:37-80); returns (alpha, residual), x updated in place."""
    dir_norm = frob_norm(direction)
    curr_alpha = alpha / change_in_alpha
    old = x.copy()
    retraction(x, direction.scaled(curr_alpha / dir_norm))
    best_res, best_alpha, best_x = calculate_residual(), curr_alpha, x.copy()
    while True:
        curr_alpha *= change_in_alpha
        assign(x, old)
        retraction(x, direction.scaled(curr_alpha / dir_norm))
        new_res = calculate_residual()
        if new_res < best_res:
            best_res, best_alpha, best_x = new_res, curr_alpha, x.copy()
        else:
            break
    assign(x, best_x)
    alpha = best_alpha
    while alpha > 1e-16 and best_res > residual - 1e-4 * alpha / dir_norm * derivative:   # armijo (:69-77)
        alpha *= change_in_alpha
        assign(x, old)
        retraction(x, direction.scaled(alpha / dir_norm))
        best_res = calculate_residual()
    return alpha, best_res


def geometric_cg(A, x: ref.TT, b: ref.TT, num_steps: int, eps: float, retraction: Callable = submanifold_retraction,
                 transport: Callable = projective_transport, spd: bool = False) -> List[float]:
    """GeometricCGVariant::solve (cg.cpp:38-124); x is updated in place (canonical, core at 0). Returns the
    residual before the first step followed by the residual after every step."""
    state = {}
    norm_b = tt_norm(b)

    def calculate_residual() -> float:
        state['res'] = _residual(A, x, b)
        return tt_norm(state['res'])

    def gradient() -> Tangent:
        if spd or A is None:
            return project(x.cores, state['res'].cores)
        return project(x.cores, ref.op_apply_cores(A, state['res'].cores, transpose=True))

    curr, last = calculate_residual(), 1e100   # (lastResidual is never updated in the reference's loop)
    hist = [curr]
    grad = gradient()
    grad_norm = frob_norm(grad)
    direction = grad.copy()
    alpha, steps = 1.0, 0
    while ((num_steps == 0 or steps < num_steps) and curr / norm_b > eps and abs(last - curr) / norm_b > eps
           and abs(1 - curr / last) / norm_b > eps):
        steps += 1
        derivative = scalar_product(grad, direction) / frob_norm(direction)
        if derivative <= 0:
            direction = grad.copy()
            derivative = frob_norm(grad)
            alpha = 1.0
        alpha, curr = line_search(x, alpha, direction, derivative, curr, retraction, calculate_residual, 0.8)
        hist.append(curr)
        old_direction = transport(x, direction)
        old_grad_norm = grad_norm
        grad = gradient()
        grad_norm = frob_norm(grad)
        beta = grad_norm / old_grad_norm   # Fletcher-Reeves update (:118)
        direction = Tangent(grad.base, [g + beta * o for g, o in zip(grad.components, old_direction.components)])
    return hist
