"""NumPy restatement of the randomized TT-SVD and of decomposition_als (helper module, not collected), of the
counter-based Gaussian matrix G(seed, stream) they draw from, and the fixtures of the tests.

    Philox4x32-10        Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11)
    randomSVD.h:31-98    the reference's randomTTSVD: sketch, RQ, project per mode, then round(ranks)
    ttNetwork.cpp:111-160   the plain TT-SVD constructor
    decompositionAls.cpp:36-65   decomposition_als

TT cores are (r_k, n_k, r_{k+1}) arrays. Everything is fp64 unless said otherwise.
"""
from typing import Callable, List, Optional, Sequence

import numpy as np

EPSILON = 8 * np.finfo(float).eps   # basic.h:51

# ---------------------------------------------------------------------------------------------- Philox4x32-10
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key) -> np.ndarray:
    """Ten rounds on counters (.., 4) and keys (.., 2) of 32-bit words (any integer arrays that broadcast);
    returns uint32 (.., 4)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]   # 32 x 32 -> 64 bits, exact in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def words(seed: int, stream: int, s: int, q: int) -> np.ndarray:
    """W(0..s-1, 0..q-1) as (s, q, 4): key = (seed low, seed high), counter = (q low, q high, i, stream)."""
    i = np.arange(s, dtype=np.uint64)[:, None]
    qq = np.arange(q, dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays(qq & np.uint64(MASK32), qq >> np.uint64(32), i, np.uint64(stream)), axis=-1)
    key = np.array([seed & MASK32, (seed >> 32) & MASK32], dtype=np.uint64)
    return philox4x32_10(ctr, key)


def normals_from_words(w: np.ndarray) -> np.ndarray:
    """(.., 4) words -> (.., 4) normals by the fp64 formula: u1 = (w0 + 1) 2^-32, u2 = w1 2^-32 give
    sqrt(-2 ln u1) cos 2 pi u2 and the same with sin; (w2, w3) likewise."""
    w = w.astype(np.float64)
    out = np.empty(w.shape)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log((w[..., a] + 1.0) * 2.0 ** -32))
        phi = 2.0 * np.pi * (w[..., a + 1] * 2.0 ** -32)
        out[..., a] = r * np.cos(phi)
        out[..., a + 1] = r * np.sin(phi)
    return out


def gaussian_matrix(seed: int, stream: int, s: int, m: int, fp32: bool = False) -> np.ndarray:
    """The leading s x m block of G(seed, stream); fp32: every normal rounded to fp32 (what a device that
    evaluates the formula in fp32 hands on, up to its intrinsics' error)."""
    q = (m + 3) // 4
    g = normals_from_words(words(seed, stream, s, q)).reshape(s, 4 * q)[:, :m]
    return g.astype(np.float32).astype(np.float64) if fp32 else g


# ---------------------------------------------------------------------------------------------- TT helpers
def tt_full(cores: Sequence[np.ndarray]) -> np.ndarray:
    out = cores[0]
    for c in cores[1:]:
        out = np.tensordot(out, c, axes=([out.ndim - 1], [0]))
    return out.reshape([c.shape[1] for c in cores])


def random_tt(dims: Sequence[int], ranks: Sequence[int], rng: np.random.Generator) -> List[np.ndarray]:
    r = [1] + list(ranks) + [1]
    return [rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))]


def rq(a: np.ndarray):
    """a = R Q with orthonormal rows of Q (min(m, n) of them)."""
    q, r = np.linalg.qr(a.T)
    return r.T, q.T


def move_core(cores: List[np.ndarray], pos: int) -> None:
    """Left-orthogonal cores before pos, right-orthogonal ones behind it (unpivoted QR / RQ sweeps)."""
    d = len(cores)
    for k in range(pos):
        a, n, b = cores[k].shape
        q, r = np.linalg.qr(cores[k].reshape(a * n, b))
        cores[k] = q.reshape(a, n, -1)
        cores[k + 1] = np.tensordot(r, cores[k + 1], axes=(1, 0))
    for k in range(d - 1, pos, -1):
        a, n, b = cores[k].shape
        r, q = rq(cores[k].reshape(a, n * b))
        cores[k] = q.reshape(-1, n, b)
        cores[k - 1] = np.tensordot(cores[k - 1], r, axes=(2, 0))


def _cut(sv: np.ndarray, max_rank: int, eps: float) -> int:
    """tensor.cpp:1463-1474: at most max_rank values, sigma_j <= eps sigma_0 dropped, at least one kept."""
    rank = min(len(sv), max_rank)
    while rank > 1 and sv[rank - 1] <= eps * sv[0]:
        rank -= 1
    return rank


def tt_round(cores: List[np.ndarray], max_ranks: Sequence[int], eps: float = EPSILON) -> List[np.ndarray]:
    """TTNetwork::round (ttNetwork.cpp:644-665): core to the right end, then the truncating sweep to 0."""
    cores = [c.copy() for c in cores]
    d = len(cores)
    move_core(cores, d - 1)
    for k in range(d - 1, 0, -1):
        a, n, b = cores[k].shape
        u, sv, vt = np.linalg.svd(cores[k].reshape(a, n * b), full_matrices=False)
        rank = _cut(sv, max_ranks[k - 1], eps)
        cores[k] = vt[:rank].reshape(rank, n, b)
        cores[k - 1] = np.tensordot(cores[k - 1], u[:, :rank] * sv[:rank], axes=(2, 0))
    return cores


def tt_svd(x: np.ndarray, max_ranks: Sequence[int], eps: float = EPSILON) -> List[np.ndarray]:
    """The TT-SVD constructor (ttNetwork.cpp:111-160): right to left, one truncated SVD per mode."""
    dims = x.shape
    d = len(dims)
    cores: List[Optional[np.ndarray]] = [None] * d
    remains = x.reshape(-1, 1)
    right = 1
    for k in range(d - 1, 0, -1):
        mat = remains.reshape(-1, dims[k] * right)
        u, sv, vt = np.linalg.svd(mat, full_matrices=False)
        rank = _cut(sv, max_ranks[k - 1], eps)
        cores[k] = vt[:rank].reshape(rank, dims[k], right)
        remains = u[:, :rank] * sv[:rank]
        right = rank
    cores[0] = remains.reshape(1, dims[0], right)
    return cores


# ---------------------------------------------------------------------------------------------- randomTTSVD
def random_ttsvd(x: np.ndarray, ranks: Sequence[int], oversampling: Sequence[int], seed: int = 0,
                 sketch: Optional[Callable[[int, int, int], np.ndarray]] = None, fp32: bool = True) -> List[np.ndarray]:
    """randomSVD.h:31-98 with the deviations of this project: s_j capped at M_j, G_j = G(seed, stream = j)
    (fp32-rounded normals by default, as the device produces them) unless `sketch(j, s, M)` supplies the matrix."""
    dims = x.shape
    d = len(dims)
    assert len(ranks) == len(oversampling) == max(d, 1) - 1 and all(r >= 1 for r in ranks)
    if d == 1:
        return [x.reshape(1, dims[0], 1).copy()]
    cores: List[Optional[np.ndarray]] = [None] * d
    b = x.reshape(-1, dims[-1])
    right = 1
    for j in range(d, 1, -1):
        M = int(np.prod(dims[:j - 1]))
        b = b.reshape(M, dims[j - 1] * right)
        s = min(ranks[j - 2] + oversampling[j - 2], M)
        G = sketch(j, s, M) if sketch is not None else gaussian_matrix(seed, j, s, M, fp32)
        _, Q = rq(G @ b)
        b = b @ Q.T
        cores[j - 1] = Q.reshape(Q.shape[0], dims[j - 1], right)
        right = Q.shape[0]
    cores[0] = b.reshape(1, dims[0], right)
    return tt_round(cores, ranks)


# ---------------------------------------------------------------------------------------------- decomposition_als
def decomposition_als(cores: List[np.ndarray], b: np.ndarray, eps: float = EPSILON, max_iterations: int = 1000):
    """decompositionAls.cpp:36-65: sweeps 0 .. d-1 then d-2 .. 1 of exact local projections; returns
    (cores, residuals) with the residual before the first and after every sweep."""
    cores = [c.copy() for c in cores]
    d = len(cores)
    dims = [c.shape[1] for c in cores]

    def project(pos):
        move_core(cores, pos)
        t = b.reshape(1, -1)
        if pos > 0:
            left = cores[0].reshape(dims[0], -1)
            for k in range(1, pos):
                left = np.tensordot(left, cores[k], axes=(left.ndim - 1, 0))
            left = left.reshape(-1, left.shape[-1])
            t = left.T @ b.reshape(left.shape[0], -1)
        if pos + 1 < d:
            right = cores[d - 1].reshape(-1, dims[d - 1])
            for k in range(d - 2, pos, -1):
                right = np.tensordot(cores[k], right, axes=(2, 0))
            right = right.reshape(right.shape[0], -1)
            t = t.reshape(-1, right.shape[1]) @ right.T
        cores[pos] = t.reshape(cores[pos].shape[0], dims[pos], -1)

    residuals = [float(np.linalg.norm(tt_full(cores) - b))]
    for _ in range(max_iterations):
        for pos in range(d):
            project(pos)
        for pos in range(d - 2, 0, -1):
            project(pos)
        residuals.append(float(np.linalg.norm(tt_full(cores) - b)))
        if residuals[-1] < EPSILON or (residuals[-2] - residuals[-1]) / residuals[-1] < eps:
            break
    return cores, residuals


# ---------------------------------------------------------------------------------------------- fixtures
EXACT_DIMS, EXACT_RANKS = (4, 5, 3, 6, 4), (3, 4, 4, 2)


def exact_rank_tensor(seed: int = 2026) -> np.ndarray:
    """The dense tensor of a random TT with EXACT_DIMS / EXACT_RANKS."""
    return tt_full(random_tt(EXACT_DIMS, EXACT_RANKS, np.random.default_rng(seed)))


def hilbert_tensor(n: int = 6, d: int = 5) -> np.ndarray:
    """Y[i_1 .. i_d] = 1 / (1 + i_1 + .. + i_d): decaying TT singular values, no exact low rank."""
    grids = np.meshgrid(*[np.arange(n)] * d, indexing="ij")
    return 1.0 / (1.0 + sum(grids))
