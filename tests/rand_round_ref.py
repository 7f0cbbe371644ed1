"""NumPy restatement of the randomized rounding of TT sums (helper module, not collected) and the fixtures of its tests.

    Al Daas, Ballard, Cazeaux, Hallman, Miedlar, Pasha, Reid, Saibaba: "Randomized algorithms for rounding in the
    tensor-train format", SISC 2023: randomize-then-orthogonalize (Alg. 3.2) on a formal sum (§3.3)
    include/xerus/algorithms/randomizedRounding.h   the recursion as this project fixes it
    xerus_amd/csrc/tt_rand.hip                      the device driver this restates

TT cores are (r_k, n_k, r_{k+1}) arrays; a term is a list of cores. The random TT Omega_k (l_k, n_k, l_{k+1}),
k = 1 .. d-1, is as a row-major l_k x (n_k l_{k+1}) matrix the leading block of G(seed, stream = k) of
random_ttsvd_ref.gaussian_matrix (fp32-rounded normals, as the device produces them), so with the same seed this
module uses the very matrix the GPU uses.
"""
from typing import Callable, List, Optional, Sequence

import numpy as np

import random_ttsvd_ref as rt

Cores = List[np.ndarray]


def capped_ranks(dims: Sequence[int], terms: Sequence[Cores], ell: Sequence[int]) -> List[int]:
    """l_0 .. l_d: ell capped, left to right, by the product of the modes on either side of the edge, by the sum of the
    terms' ranks and by l_{k-1} n_{k-1}; l_0 = l_d = 1."""
    d = len(dims)
    l = [1] * (d + 1)
    for k in range(1, d):
        left = int(np.prod([int(x) for x in dims[:k]], dtype=object))
        right = int(np.prod([int(x) for x in dims[k:]], dtype=object))
        total = sum(t[k].shape[0] for t in terms)
        l[k] = min(int(ell[k - 1]), left, right, total, l[k - 1] * dims[k - 1])
    return l


def omega(seed: int, k: int, lk: int, nk: int, lk1: int, fp32: bool = True) -> np.ndarray:
    return rt.gaussian_matrix(seed, k, lk, nk * lk1, fp32).reshape(lk, nk, lk1)


def sketch_sum(terms: Sequence[Cores], coef: Sequence[float], ell: Sequence[int], seed: int = 0,
               random_core: Optional[Callable[[int, int, int, int], np.ndarray]] = None, fp32: bool = True) -> Cores:
    """The two passes: the rank-l sketch result of sum_j coef[j] terms[j], cores 0 .. d-2 left-orthonormal, the core at
    d - 1. random_core(k, l_k, n_k, l_{k+1}) replaces G(seed, stream = k) when given."""
    dims = [c.shape[1] for c in terms[0]]
    d = len(dims)
    assert len(coef) == len(terms) and all([c.shape[1] for c in t] == dims for t in terms)
    if d == 1:
        return [sum(c * t[0] for c, t in zip(coef, terms))]
    assert len(ell) == d - 1 and all(e >= 1 for e in ell)
    l = capped_ranks(dims, terms, ell)
    # pass 1, right to left, each term on its own
    W = [[None] * (d + 1) for _ in terms]
    for k in range(d - 1, 0, -1):
        om = random_core(k, l[k], dims[k], l[k + 1]) if random_core is not None else omega(seed, k, l[k], dims[k], l[k + 1], fp32)
        H = om.reshape(l[k], dims[k] * l[k + 1])
        for j, t in enumerate(terms):
            Wn = W[j][k + 1] if k + 1 < d else np.ones((1, 1))
            T = np.tensordot(t[k], Wn, axes=(2, 0))                # (R_k, n_k, l_{k+1})
            W[j][k] = T.reshape(T.shape[0], -1) @ H.T               # (R_k, l_k)
    # pass 2, left to right
    out: Cores = [None] * d
    X = [c * t[0] for c, t in zip(coef, terms)]
    for k in range(d - 1):
        Z = sum(x.reshape(l[k] * dims[k], -1) @ W[j][k + 1] for j, x in enumerate(X))
        Q, _ = np.linalg.qr(Z)
        out[k] = Q.reshape(l[k], dims[k], l[k + 1])
        M = [Q.T @ x.reshape(l[k] * dims[k], -1) for x in X]
        X = [np.tensordot(m, t[k + 1], axes=(1, 0)) for m, t in zip(M, terms)]
    out[d - 1] = sum(X)
    return out


def sum_rounded(terms: Sequence[Cores], coef: Sequence[float], ranks: Sequence[int], oversampling: Sequence[int],
                seed: int = 0, **kw) -> Cores:
    """sketch_sum at l_k = ranks[k] + oversampling[k], then the deterministic round(ranks)."""
    cores = sketch_sum(terms, coef, [r + p for r, p in zip(ranks, oversampling)], seed, **kw)
    return rt.tt_round(cores, ranks) if len(cores) > 1 else cores


def block_sum(terms: Sequence[Cores], coef: Sequence[float]) -> Cores:
    """The block-diagonal cores of sum_j coef[j] terms[j] (what operator+ writes), coefficients in the first core."""
    d = len(terms[0])
    if d == 1:
        return [sum(c * t[0] for c, t in zip(coef, terms))]
    out = []
    for k in range(d):
        n = terms[0][k].shape[1]
        if k == 0:
            out.append(np.concatenate([c * t[0] for c, t in zip(coef, terms)], axis=2))
        elif k == d - 1:
            out.append(np.concatenate([t[k] for t in terms], axis=0))
        else:
            ra, rb = [t[k].shape[0] for t in terms], [t[k].shape[2] for t in terms]
            blk = np.zeros((sum(ra), n, sum(rb)))
            a = b = 0
            for t, x, y in zip(terms, ra, rb):
                blk[a:a + x, :, b:b + y] = t[k]
                a, b = a + x, b + y
            out.append(blk)
    return out


def full_sum(terms: Sequence[Cores], coef: Sequence[float]) -> np.ndarray:
    return sum(c * rt.tt_full(t) for c, t in zip(coef, terms))


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------------------- fixtures
DIMS = (6, 5, 4, 5, 6)
Z_RANKS, U_RANKS, NOISE_RANKS = (6, 7, 7, 6), (5, 5, 5, 5), (6, 9, 9, 6)


def exact_fixture(seed: int = 2027):
    """(terms, coefficients, exact ranks): z, 2.5 u, -2.5 u, whose sum is z of ranks Z_RANKS."""
    rng = np.random.default_rng(seed)
    z, u = rt.random_tt(DIMS, Z_RANKS, rng), rt.random_tt(DIMS, U_RANKS, rng)
    return [z, u, [c.copy() for c in u]], [1.0, 2.5, -2.5], list(Z_RANKS)


def noisy_fixture(seed: int = 2028):
    """(terms, coefficients, ranks): z + 1e-3 ||z|| (a / ||a|| + b / ||b||) with a, b of ranks NOISE_RANKS, to be
    rounded to Z_RANKS."""
    rng = np.random.default_rng(seed)
    z, a, b = rt.random_tt(DIMS, Z_RANKS, rng), rt.random_tt(DIMS, NOISE_RANKS, rng), rt.random_tt(DIMS, NOISE_RANKS, rng)
    nz = np.linalg.norm(rt.tt_full(z))
    return [z, a, b], [1.0, 1e-3 * nz / np.linalg.norm(rt.tt_full(a)), 1e-3 * nz / np.linalg.norm(rt.tt_full(b))], list(Z_RANKS)


def ragged_fixture(seed: int = 2029):
    """(terms, coefficients, sketch ranks): term ranks (2,3,2,2), (5,5,5,5), (1,1,1,1), one coefficient 0, one mode of
    size 1. The sketch ranks stay below the exact ranks of the sum's unfoldings, so every Z has full rank."""
    dims = (4, 5, 1, 6, 3)
    rng = np.random.default_rng(seed)
    terms = [rt.random_tt(dims, (2, 3, 2, 2), rng), rt.random_tt(dims, (5, 5, 5, 5), rng), rt.random_tt(dims, (1, 1, 1, 1), rng)]
    return terms, [1.5, 0.0, -0.75], [3, 3, 3, 3]
