"""NumPy restatement of the reference's UQ-ADF (src/xerus/algorithms/uqAdf.cpp; helper module, not collected).

    uqAdf.cpp:40-52     randVar_to_position
    uqAdf.cpp:110-282   InternalSolver: left / right stacks, delta, ||A(delta)||, residual
    uqAdf.cpp:285-322   InternalSolver::solve
    uqAdf.cpp:334-411   uq_adf(UQMeasurementSet, guess) with its initialisation from initial measurements
    uqAdf.cpp:425-477   uq_mc, uq_avg

It builds on oracle.xerus_ref for the TT operations of the reference (move_core with keepRank, sums, round) and
its random stream. TT cores are (r_k, n_k, r_{k+1}) arrays. The reference loops over the N samples one by one;
here every per-sample contraction is one einsum over the sample axis j, the same products in the same
association order.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import xerus_ref as ref


def hermite(v, n: int) -> np.ndarray:
    """randVar_to_position (:40-52): boost::math::hermite(i, v / sqrt 2) / 2^(i/2), i.e. the probabilists'
    Hermite polynomials He_0 = 1, He_1 = v, He_{i+1} = v He_i - i He_{i-1}. v scalar or (N,): (n,) or (N, n)."""
    v = np.asarray(v, dtype=np.float64)
    p = np.empty(v.shape + (n,))
    if n > 0:
        p[..., 0] = 1.0
    if n > 1:
        p[..., 1] = v
    for i in range(1, n - 1):
        p[..., i + 1] = v * p[..., i] - i * p[..., i - 1]
    return p


def positions(dims: Sequence[int], rv: np.ndarray) -> List[Optional[np.ndarray]]:
    """create_positions (:72-83): P[k] (N x n_k) for k >= 1."""
    return [None] + [hermite(rv[:, k - 1], dims[k]) for k in range(1, len(dims))]


def evaluate(x: ref.TT, rv: np.ndarray) -> np.ndarray:
    """The sample loop of uq_mc (:436-444): N x n_0 solutions of x at the random vectors rv (N x d-1)."""
    N, d = rv.shape[0], x.order
    p = np.ones((N, 1))
    for k in range(d - 1, 0, -1):
        t = np.einsum('atb,jb->jat', x.cores[k], p)                              # :439
        p = np.einsum('jat,jt->ja', t, hermite(rv[:, k - 1], x.dims[k]))          # :440
    return np.einsum('nb,jb->jn', x.cores[0][0], p)                              # :442


def make_case(dims: Sequence[int], ranks: Sequence[int], N: int, seed: int):
    """The recipe of the test cases: (target, random vectors N x d-1, the target's solutions there, start)."""
    rng = ref.Rng(seed)
    true = ref.TT.random(dims, ranks, rng)
    rv = np.random.default_rng(seed).standard_normal((N, len(dims) - 1))
    sols = evaluate(true, rv)
    x0 = ref.TT.random(dims, ranks, rng)
    return true, rv, sols, x0


# dims / ranks / N / seed. Each converges in the restatement to a residual <= 3e-15 within 1000 iterations; other
# seeds at these shapes stall above 1e-8 here too.
FULL_SOLVE_CASES = [
    ([5, 3], [2], 40, 3),
    ([5, 3, 4], [2, 3], 64, 4),
    ([7, 4, 1, 3], [3, 1, 1], 50, 5),
    ([33, 4, 3], [12, 3], 130, 8),
]


def _measured(P, C):
    """measCmp (:128): M_j = sum_t P[j, t] C[:, t, :]."""
    return np.einsum('jt,atb->jab', P, C)


def uq_adf(x: ref.TT, rv: np.ndarray, sols: np.ndarray, max_iterations: int = 1000) -> List[float]:
    """InternalSolver::solve (:285-322) on x in place; returns the relative residuals (one per iteration, the
    stopping one included). The reference hard-codes max_iterations = 1000."""
    rv = np.asarray(rv, dtype=np.float64)
    S = np.asarray(sols, dtype=np.float64)
    N, d = rv.shape[0], x.order
    P = positions(x.dims, rv)
    snorm = np.sqrt(np.sum(S * S))                                               # :85-92
    residuals = [1000.0] * 10                                                    # :286
    for _ in range(max_iterations):
        x.move_core(0, True)                                                     # :290
        R: List[Optional[np.ndarray]] = [None] * (d + 1)
        for k in range(d - 1, 0, -1):                                            # :293-295, calc_right_stack :143-161
            M = _measured(P[k], x.cores[k])
            R[k] = M[:, :, 0] if k == d - 1 else np.einsum('jab,jb->ja', M, R[k + 1])
        left_is: List[Optional[np.ndarray]] = [None] * d
        left_ought: List[Optional[np.ndarray]] = [None] * d
        for k in range(d):
            if k == 0:
                X0 = x.cores[0][0]                                               # n_0 x r_1
                residuals.append(float(np.linalg.norm(R[1] @ X0.T - S)) / snorm)  # :268-282, :300
                if residuals[-1] / residuals[-10] > 0.99:                        # :302
                    return residuals[10:]
                delta = ((R[1] @ X0.T - S).T @ R[1])[None, :, :]                 # :204-217
                norm_a = np.sqrt(np.sum((R[1] @ delta[0].T) ** 2))               # :227-233
            else:
                Rn = R[k + 1] if k < d - 1 else np.ones((N, 1))
                is_part = np.einsum('jab,jb->ja', _measured(P[k], x.cores[k]), Rn)   # :185-191
                if k > 1:
                    is_part = np.einsum('jac,jc->ja', left_is[k - 1], is_part)   # :193-195
                e = is_part - left_ought[k - 1]
                delta = np.einsum('ja,jt,jb->atb', e, P[k], Rn)                  # :176-180, :199-202
                g = np.einsum('jab,jb->ja', _measured(P[k], delta), Rn)          # :244-250
                if k > 1:
                    norm_a = np.sqrt(np.einsum('ja,jac,jc->', g, left_is[k - 1], g))   # :252-254
                else:
                    norm_a = np.sqrt(np.sum(g * g))                              # :256
            pyr = float(np.sum(delta * delta))                                   # :310
            x.cores[k] = x.cores[k] - (pyr / norm_a ** 2) * delta                # :313
            if k + 1 < d:
                x.move_core(k + 1, True)                                         # :317
                if k == 0:                                                       # calc_left_stack :113-121
                    left_ought[0] = S @ x.cores[0][0]
                else:                                                            # :123-139
                    M = _measured(P[k], x.cores[k])
                    if k > 1:
                        left_is[k] = np.einsum('jca,jcd,jdb->jab', M, left_is[k - 1], M)
                    else:
                        left_is[k] = np.einsum('jca,jcb->jab', M, M)
                    left_ought[k] = np.einsum('ja,jab->jb', left_ought[k - 1], M)
    return residuals[10:]


def _dirac_core(n: int, pos: int) -> np.ndarray:
    c = np.zeros((1, n, 1))
    c[0, pos, 0] = 1.0
    return c


def _zero_tt(dims: Sequence[int]) -> ref.TT:
    """TTTensor(dimensions) (ttNetwork.cpp:104-105): dirac components, the first one zero; core at 0."""
    cores = [_dirac_core(n, 0) for n in dims]
    cores[0][0, 0, 0] = 0.0
    return ref.TT(cores, True, 0)


def _add(x: ref.TT, y: ref.TT) -> ref.TT:
    """TTNetwork::operator+= on a canonicalised x (ttNetwork.cpp:797-847): block cores, then move_core back."""
    z = ref.tt_add(x, y)
    z.move_core(x.core_position)
    return z


def uq_adf_initial(dims: Sequence[int], rv, sols, init_rv, init_sols) -> ref.TT:
    """The starting point of uq_adf(UQMeasurementSet, guess) with initial measurements (:338-403): a mean term
    (the mean over `sols` only, :346-351) plus one linear term per stochastic mode, rounded at 0.00025."""
    sols = np.asarray(sols, dtype=np.float64)
    init_rv = np.asarray(init_rv, dtype=np.float64)
    init_sols = np.asarray(init_sols, dtype=np.float64)
    d = len(dims)
    assert init_rv.shape == (d - 1, d - 1) and init_sols.shape[0] == d - 1                  # :365-367
    mean = sols.sum(axis=0) / float(len(sols))
    new_x = _zero_tt(dims)
    base = [mean.reshape(1, dims[0], 1)] + [_dirac_core(dims[k + 1], 0) for k in range(d - 1)]   # :353-360
    new_x = _add(new_x, ref.TT(base, True, 0))
    for m in range(d - 1):                                                                  # :369-386
        assert init_rv[m, m] > 0.0
        cores = [(init_sols[m] - mean).reshape(1, dims[0], 1)]
        for k in range(d - 1):
            assert k == m or init_rv[m, k] == 0.0
            cores.append(_dirac_core(dims[k + 1], 0 if k == m else 1))
        new_x = _add(new_x, ref.TT(cores, True, 0))
    new_x.round(2 ** 62, 0.00025)                                                           # :402
    return new_x


def uq_adf_measurements(guess: ref.TT, rv, sols, init_rv=None, init_sols=None, max_iterations: int = 1000) -> Tuple[ref.TT, List[float]]:
    """uq_adf(UQMeasurementSet, guess) (:334-411). The solver gets the unmerged measurements (:404)."""
    if init_rv is not None and len(init_rv) > 0:
        x = uq_adf_initial(guess.dims, rv, sols, init_rv, init_sols)
    else:
        x = guess.copy()
    hist = uq_adf(x, np.asarray(rv), np.asarray(sols), max_iterations)
    return x, hist


def uq_mc(x: ref.TT, N: int, num_special: int, rng: Optional[ref.Rng] = None) -> Tuple[np.ndarray, np.ndarray]:
    """uq_mc (:425-448): a default-seeded std::mt19937_64 (5489), one normal per (sample, k) with k running
    from d-1 down to 1, scaled by 0.3 for k <= numSpecial."""
    rng = rng or ref.Rng(5489)
    d = x.order
    draws = rng.normal(N * (d - 1)).reshape(N, d - 1)[:, ::-1]      # column k-1 = the draw for mode k
    scale = np.array([0.3 if k <= num_special else 1.0 for k in range(1, d)])
    rv = np.ascontiguousarray(draws * scale[None, :])
    return rv, evaluate(x, rv)


def uq_avg(x: ref.TT, N: int, num_special: int) -> np.ndarray:
    """uq_avg (:451-477) without OpenMP: the mean of uq_mc's solutions."""
    return uq_mc(x, N, num_special)[1].sum(axis=0) / float(N)
