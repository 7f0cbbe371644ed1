"""NumPy restatement of the reference's find_largest_entry (src/xerus/algorithms/largestEntry.cpp:6-54; helper
module, not collected), the closed-form symmetric-square cores of DESIGN §3.8, and the fixtures of the tests.

    largestEntry.cpp:10-36   the power iteration: X o X, soft_threshold, round(1), normalise
    largestEntry.cpp:38-53   the rank-one branch: per component the first index of largest modulus

It builds on oracle.xerus_ref.TT for move_core, soft_threshold, round and frob_norm. TT cores are
(r_k, n_k, r_{k+1}) arrays.
"""
from typing import Callable, List, Sequence, Tuple

import numpy as np

from oracle import xerus_ref as ref

SQRT2 = np.sqrt(2.0)


# ---------------------------------------------------------------------------------------------- the two squares
def kronecker_square(x: ref.TT) -> ref.TT:
    """entrywise_product(X, X) (ttNetwork.cpp:1275-1309): cores X_k[i] (x) X_k[i] of rank r^2, moved to the core
    position when X is canonical (:1303-1306)."""
    cores = []
    for c in x.cores:
        a, n, b = c.shape
        cores.append(np.einsum('aib,cid->acibd', c, c).reshape(a * a, n, b * b))
    z = ref.TT(cores)
    if x.canonicalized:
        z.move_core(x.core_position)
    return z


def sym_rank(r: int) -> int:
    return r * (r + 1) // 2


def pair_index(a: int, b: int, r: int) -> int:
    """p(a, b) = a r - a (a - 1) / 2 + (b - a), 0 <= a <= b < r."""
    return a * r - a * (a - 1) // 2 + (b - a)


def pairs(r: int) -> List[Tuple[int, int]]:
    """(a, b) in the order of the pair index."""
    return [(a, b) for a in range(r) for b in range(a, r)]


def symmetric_square_core(A: np.ndarray) -> np.ndarray:
    """C[p(a,b), i, p(a',b')] of the table in DESIGN §3.8, entry by entry (the expected values of the kernel):
    A[a,i,a']^2 | sqrt 2 A[a,i,a'] A[a,i,b'] | sqrt 2 A[a,i,a'] A[b,i,a'] | A[a,i,a'] A[b,i,b'] + A[a,i,b'] A[b,i,a']."""
    ra, n, rb = A.shape
    C = np.empty((sym_rank(ra), n, sym_rank(rb)))
    for p, (a, b) in enumerate(pairs(ra)):
        for q, (a2, b2) in enumerate(pairs(rb)):
            if a == b and a2 == b2:
                C[p, :, q] = A[a, :, a2] * A[a, :, a2]
            elif a == b:
                C[p, :, q] = SQRT2 * (A[a, :, a2] * A[a, :, b2])
            elif a2 == b2:
                C[p, :, q] = SQRT2 * (A[a, :, a2] * A[b, :, a2])
            else:
                C[p, :, q] = A[a, :, a2] * A[b, :, b2] + A[a, :, b2] * A[b, :, a2]
    return C


def symmetric_square_scale(A: np.ndarray) -> np.ndarray:
    """Per entry of symmetric_square_core the largest |product of two core entries| involved (the scale of its
    rounding-error bar)."""
    ra, n, rb = A.shape
    S = np.empty((sym_rank(ra), n, sym_rank(rb)))
    for p, (a, b) in enumerate(pairs(ra)):
        for q, (a2, b2) in enumerate(pairs(rb)):
            S[p, :, q] = np.maximum(np.abs(A[a, :, a2] * A[b, :, b2]), np.abs(A[a, :, b2] * A[b, :, a2]))
    return S


def symmetric_square(x: ref.TT) -> ref.TT:
    """X o X with the closed-form cores (ranks r (r + 1) / 2), moved to the core position when X is canonical."""
    z = ref.TT([symmetric_square_core(c) for c in x.cores])
    if x.canonicalized:
        z.move_core(x.core_position)
    return z


# ---------------------------------------------------------------------------------------------- the algorithm
def entry(x: ref.TT, position: int) -> float:
    """_T[position] (row-major over the dimensions)."""
    idx = np.unravel_index(position, x.dims)
    v = np.ones((1,))
    for c, i in zip(x.cores, idx):
        v = v @ c[:, i, :]
    return float(v[0])


def rank_one_position(x: ref.TT) -> int:
    """:38-53 for a TTTensor: the strict > scan keeps the first index of largest modulus."""
    position = 0
    for c in x.cores:
        v = c.reshape(-1)                       # (1, n, 1)
        max_pos = 0
        for i in range(1, v.size):              # :46
            if abs(v[i]) > abs(v[max_pos]):     # :47
                max_pos = i
        position = position * v.size + max_pos  # :43, :51
    return position


def find_largest_entry(t: ref.TT, accuracy: float, lower_bound: float = 0.0,
                       square: Callable[[ref.TT], ref.TT] = kronecker_square, max_iterations: int = 1000,
                       trace: list | None = None) -> int:
    """largestEntry.cpp:6-54 for a TTTensor. `square` forms X o X (:20): the Kronecker cores of the reference or
    the symmetric-square cores. trace, when given, receives the largest rank before the threshold per iteration."""
    d = t.order
    if sum(t.ranks) >= d:                                                       # :10
        alpha = accuracy                                                        # :11
        x = t.copy()                                                            # :13
        x.round(1)                                                              # :14
        xn = max(entry(t, find_largest_entry(x, 0.0, 0.0)), lower_bound)        # :15
        tau = (1 - alpha) * alpha * xn * xn / (2.0 * (d - 1))                   # :16
        x = t.copy()                                                            # :18
        it = 0
        while sum(x.ranks) >= d:                                                # :19
            it += 1
            if it > max_iterations:
                raise RuntimeError("no rank-one iterate after %d iterations" % max_iterations)
            x = square(x)                                                       # :20
            if trace is not None:
                trace.append(max(x.ranks))
            x.soft_threshold(tau)                                               # :22
            y = x.copy()                                                        # :24
            y.round(1)                                                          # :25
            y_max_pos = find_largest_entry(y, 0.0, 0.0)                         # :26
            xn = max(entry(x, y_max_pos), (1 - (1 - alpha) * alpha / 2.0) * xn * xn)   # :28
            f_norm = x.frob_norm()                                              # :30
            if not (np.isfinite(f_norm) and f_norm > 0.0):
                raise RuntimeError("norm of the iterate is zero or not finite")
            xn /= f_norm                                                        # :31
            k = x.core_position if x.canonicalized else 0
            x.cores[k] = x.cores[k] / f_norm                                    # :32
            tau = (1 - alpha) * alpha * xn * xn / (2.0 * (d - 1))               # :33
        return rank_one_position(x)                                             # :35
    return rank_one_position(t)                                                 # :37-53


# ---------------------------------------------------------------------------------------------- fixtures
# (dims, ranks, seed): TT.random(dims, ranks, Rng(seed)) divided by its Frobenius norm, as the reference's unit test
# (src/unitTests/largestEntry.cxx:28-76). The calls use accuracy = the gap ratio and lowerBound = |largest|.
FIXTURES = [
    ([2] * 10, [3] * 9, 3),
    ([2] * 10, [3] * 9, 6),
    ([3, 2, 3, 2, 3, 2, 3, 2], [4] * 7, 1),
    ([3, 2, 3, 2, 3, 2, 3, 2], [4] * 7, 4),
    ([5, 7], [4], 2),
    ([5, 7], [4], 4),
    ([3] * 6, [1] * 5, 1),   # the rank-one branch
    ([9], [], 2),            # d = 1 (an exact scan; the seed gives a negative largest entry at the last index)
]
FIXTURE_IDS = ["%s-r%s-s%d" % ("x".join(map(str, d)), (r[0] if r else 0), s) for d, r, s in FIXTURES]


def make_fixture(dims: Sequence[int], ranks: Sequence[int], seed: int) -> ref.TT:
    x = ref.TT.random(list(dims), list(ranks), ref.Rng(seed))
    nrm = x.frob_norm()
    x.cores[x.core_position] = x.cores[x.core_position] / nrm
    return x


def gap(full: np.ndarray) -> Tuple[int, float, float]:
    """(argmax |full|, the largest entry with its sign, |second largest| / |largest|)."""
    flat = np.abs(full).ravel()
    order = np.argsort(-flat, kind="stable")
    pos = int(order[0])
    second = flat[order[1]] if flat.size > 1 else 0.0
    return pos, float(full.ravel()[pos]), float(second / flat[pos])
