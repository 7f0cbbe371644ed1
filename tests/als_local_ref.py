"""numpy restatement of the matrix-free ALS local problem (xerus_amd/csrc/als_local.hip): both GEMM chains by
reshapes and `@`, the conjugate-gradient iteration with its freeze semantics, the environments of a site, and the
three-site test problems shared by the CPU and the GPU tests."""
import functools

import numpy as np

# (rl, n, rr, pl, pr): two boundary sites below one wave, odd extents with unequal operator ranks, operator
# rank 1, and N = 4092 (several blocks with a ragged tail)
SHAPES = [(1, 3, 2, 1, 2), (7, 4, 1, 3, 1), (5, 3, 7, 2, 3), (16, 5, 16, 1, 1), (33, 4, 31, 2, 2)]
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------- the operator
def apply_einsum(x, L, A, R, normal):
    """y = M x, the definition (include/xerus_amd.h)."""
    if normal:
        return np.einsum('apqc,pyis,qyjt,bstd,cjd->aib', L, A, A, R, x, optimize=True)
    return np.einsum('apc,pijq,bqd,cjd->aib', L, A, R, x, optimize=True)


def dense_operator(L, A, R, normal):
    """M as an N x N matrix, N = rl n rr (the tensor construct_local_operator assembles)."""
    if normal:
        M = np.einsum('apqc,pyis,qyjt,bstd->aibcjd', L, A, A, R, optimize=True)
    else:
        M = np.einsum('apc,pijq,bqd->aibcjd', L, A, R, optimize=True)
    N = M.shape[0] * M.shape[1] * M.shape[2]
    return M.reshape(N, N)


def contraction_lengths(dims, normal):
    """K of every GEMM of the chain."""
    rl, n, rr, pl, pr = dims
    return [rl, pl * n, pl * n, pr * pr * rr] if normal else [rl, pl * n, pr * rr]


def apply_chain(x, L, A, R, normal):
    """y = M x as the kernel computes it: plain matrix products of reshaped operands; the only permutation is
    Ahat[(p,j),(i,q)] = A(p,i,j,q)."""
    rl, n, rr = x.shape
    pl, pr = A.shape[0], A.shape[3]
    Ahat = np.ascontiguousarray(A.transpose(0, 2, 1, 3)).reshape(pl * n, n * pr)
    X = x.reshape(rl, n * rr)
    if not normal:
        T1 = L.reshape(rl * pl, rl) @ X                                   # [(a,p),(j,b')]
        T1 = T1.reshape(rl, pl * n, rr)
        T2 = np.stack([Ahat.T @ T1[a] for a in range(rl)])                # per a: [(i,q),b']
        return (T2.reshape(rl * n, pr * rr) @ R.reshape(rr, pr * rr).T).reshape(rl, n, rr)
    T1 = L.reshape(rl * pl * pl, rl) @ X                                  # [(a,p,p'),(j,b')]
    T1 = T1.reshape(rl * pl, pl * n, rr)
    T2 = np.stack([Ahat.T @ T1[i] for i in range(rl * pl)])               # per (a,p): [(y,q'),b']
    T2 = T2.reshape(rl, pl * n, pr * rr)                                  # per a: [(p,y),(q',b')]
    An = A.reshape(pl * n, n * pr)                                        # [(p,y),(i,q)]
    T3 = np.stack([An.T @ T2[a] for a in range(rl)])                      # per a: [(i,q),(q',b')]
    return (T3.reshape(rl * n, pr * pr * rr) @ R.reshape(rr, pr * pr * rr).T).reshape(rl, n, rr)


# ------------------------------------------------------------------------------------------- CG
CONVERGED, MAX_ITER, BREAKDOWN = 0, 1, 2


def cg(matvec, x0, b, tol, max_iter=0, check_every=1):
    """xrs_als_local_cg restated: plain CG from x0; the device state (done, skip, status, iters) is updated every
    iteration, the host looks at `done` every check_every iterations, and a frozen iteration changes nothing.
    Returns (x, iters, relres, status)."""
    N = b.size
    cap = 4 * N + 50
    if max_iter == 0 or max_iter > cap:
        max_iter = cap
    x = np.array(x0, dtype=np.float64)
    r = b - matvec(x)
    p = r.copy()
    rr, bb = float(np.sum(r * r)), float(np.sum(b * b))
    if bb == 0.0:
        return np.zeros_like(x), 0, 0.0, CONVERGED
    thresh = tol * tol * bb
    done, status, iters = rr <= thresh, CONVERGED, 0
    seen, k = done, 0
    while k < max_iter and not seen:
        q = matvec(p)
        pq = float(np.sum(p * q))
        # (ii)
        if done:
            skip = True
        elif not pq > 0.0 or not np.isfinite(pq):
            status, skip = BREAKDOWN, True
        else:
            alpha = rr / pq
            x += alpha * p
            r -= alpha * q
            skip = False
        # (iii)
        if skip:
            done = True
        else:
            rrn = float(np.sum(r * r))
            p = r + (rrn / rr) * p
            rr = rrn
            iters += 1
            if rrn <= thresh:
                done = True
        k += 1
        if k % check_every == 0 or k == max_iter:
            seen = done
    return x, iters, float(np.sqrt(rr / bb)), (status if done else MAX_ITER)


# ------------------------------------------------------------------------------------------- environments
def environments(op_cores, x_cores, site, normal):
    """(L, R) of `site`: the stacks of ALS (oracle/xerus_ref.py: op_left / op_right) contracted up to it. Symmetric
    form: L (rl, pl, rl), R (rr, pr, rr); normal: L (rl, pl, pl, rl), R (rr, pr, pr, rr)."""
    d = len(x_cores)
    L = np.ones((1, 1, 1, 1)) if normal else np.ones((1, 1, 1))
    R = L.copy()
    for k in range(site):
        X, Ak = x_cores[k], op_cores[k]
        if normal:
            L = np.einsum('pqrs,pnc,qmnd,rmle,slf->cdef', L, X, Ak, Ak, X, optimize=True)
        else:
            L = np.einsum('pqr,pnc,qnmd,rme->cde', L, X, Ak, X, optimize=True)
    for k in range(d - 1, site, -1):
        X, Ak = x_cores[k], op_cores[k]
        if normal:
            R = np.einsum('pnc,qmnd,rmle,slf,cdef->pqrs', X, Ak, Ak, X, R, optimize=True)
        else:
            R = np.einsum('pnc,qnmd,rme,cde->pqr', X, Ak, X, R, optimize=True)
    return L, R


# ------------------------------------------------------------------------------------------- test problems
def laplace_core(n, pl, pr, shift):
    """The Laplace operator's TT core (I / T / I pattern, T = tridiag(-1, 2, -1) + shift) at operator ranks
    (pl, pr): where a bond has rank >= 2 its first two indices carry the Kronecker sum, further indices are empty;
    a bond of rank 1 cuts the sum there (the operator is the Kronecker product of the two sides' Laplacians). With
    shift > 0 every such operator is symmetric positive definite."""
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1) + shift * np.eye(n)
    I = np.eye(n)
    c = np.zeros((pl, n, n, pr))
    if pl >= 2 and pr >= 2:
        c[0, :, :, 0], c[1, :, :, 0], c[1, :, :, 1] = I, T, I
    elif pl >= 2:
        c[0, :, :, 0], c[1, :, :, 0] = I, T
    elif pr >= 2:
        c[0, :, :, 0], c[0, :, :, 1] = T, I
    else:
        c[0, :, :, 0] = T
    return c


def random_operands(dims, normal, seed):
    """Random x, L, A, R of the extents dims (no structure: for the product alone)."""
    rl, n, rr, pl, pr = dims
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rl, n, rr))
    A = rng.standard_normal((pl, n, n, pr))
    if normal:
        return x, rng.standard_normal((rl, pl, pl, rl)), A, rng.standard_normal((rr, pr, pr, rr))
    return x, rng.standard_normal((rl, pl, rl)), A, rng.standard_normal((rr, pr, rr))


class Problem:
    """A three-site problem with the middle site active: operator cores, orthonormal outer x cores, and the local
    system M x = b of the middle site with its dense restatement."""

    def __init__(self, dims, normal, seed=5):
        rl, n, rr, pl, pr = dims
        self.dims, self.normal = dims, normal
        rng = np.random.default_rng(seed + 97 * sum(dims) + int(normal))
        ns = [rl, n, rr]   # the smallest outer mode sizes at which the outer cores can be orthonormal
        ranks = [1, pl, pr, 1]
        # shifts: across a bond of rank 1 the factors' condition numbers multiply (and square in the normal form);
        # with T's spectrum in [1, 5] / [2, 6] kappa(M) stays below ~1e3 at every shape
        cores = [laplace_core(ns[k], ranks[k], ranks[k + 1], 2.0 if normal else 1.0) for k in range(3)]
        if normal:   # the perturbed non-symmetric cores of the ALS oracle test, plus weight on the empty rank slices
            cores = [c + 0.1 * rng.standard_normal(c.shape) * (c != 0) + 0.02 * rng.standard_normal(c.shape) for c in cores]
        else:        # a symmetric perturbation of every slice
            pert = [0.02 * rng.standard_normal(c.shape) for c in cores]
            cores = [c + 0.5 * (e + e.transpose(0, 2, 1, 3)) for c, e in zip(cores, pert)]
        self.op_cores = cores
        Q0 = np.linalg.qr(rng.standard_normal((rl, rl)))[0]
        Q2 = np.linalg.qr(rng.standard_normal((rr, rr)))[0]
        self.x_cores = [Q0.reshape(1, rl, rl), rng.standard_normal((rl, n, rr)), Q2.reshape(rr, rr, 1)]
        self.L, self.R = environments(cores, self.x_cores, 1, normal)
        self.A = cores[1]
        self.b = rng.standard_normal((rl, n, rr))
        self.x0 = self.x_cores[1]
        self.N = rl * n * rr

    def matvec(self, v):
        return apply_chain(v, self.L, self.A, self.R, self.normal)

    @functools.cached_property
    def M(self):
        return dense_operator(self.L, self.A, self.R, self.normal)

    @functools.cached_property
    def eigenvalues(self):
        return np.linalg.eigvalsh(0.5 * (self.M + self.M.T))

    @property
    def kappa(self):
        return float(self.eigenvalues[-1] / self.eigenvalues[0])

    @functools.cached_property
    def solution(self):
        return np.linalg.solve(self.M, self.b.reshape(self.N)).reshape(self.b.shape)

    def check_solution(self, x, relres, tol):
        """The bars of the CG tests: returned relres <= tol, true residual <= 2 tol, error <= 2 kappa tol."""
        nb = np.linalg.norm(self.b)
        true_res = np.linalg.norm(self.b.reshape(self.N) - self.M @ x.reshape(self.N)) / nb
        err = np.linalg.norm(x - self.solution) / np.linalg.norm(self.solution)
        print("dims %s normal %d: kappa %.3e relres %.3e true residual %.3e error %.3e" %
              (self.dims, self.normal, self.kappa, relres, true_res, err))
        assert relres <= tol, relres
        assert true_res <= 2 * tol, true_res
        assert err <= 2 * self.kappa * tol, (err, self.kappa)


@functools.lru_cache(maxsize=None)
def problem(dims, normal):
    """One shared, unchanged Problem per case."""
    return Problem(dims, normal)
