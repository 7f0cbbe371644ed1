"""numpy restatement of the matrix-free eigen sweep (xerus_amd/csrc/als_eig.hip, host/als_eigen.cpp): the 3 x 3
generalised eigenproblem of the LOBPCG step with its pivot rule (geneig_lowest), the iteration with its freeze
semantics and statuses (lobpcg), and the single-site sweep with QR core moves (sweep). The local problems and the
environments are those of tests/als_local_ref.py."""
import math

import numpy as np

import als_local_ref as lr

CONVERGED, MAX_ITER, BREAKDOWN = 0, 1, 2
PIVOT_MIN = 1e-8       # smallest admitted squared Cholesky pivot of the unit-diagonal Gram matrix (geneig.hpp)
JACOBI_SWEEPS = 10
JACOBI_SKIP = 1e-20


# ------------------------------------------------------------------------------------------- the small problem
def _unpack(k, t):
    m = np.zeros((k, k))
    m[np.triu_indices(k)] = t[:k * (k + 1) // 2]
    return m + np.triu(m, 1).T


def _geneig_try(k, g, h):
    """The smallest pair of the leading k x k pencil, or None (a pivot below PIVOT_MIN, or a value that is not
    finite). Same operations in the same order as geneig_try (geneig.hpp)."""
    d = np.zeros(3)
    for i in range(k):
        if not g[i, i] > 0.0:
            return None
        d[i] = 1.0 / math.sqrt(g[i, i])
    gs = np.array([[g[i, j] * d[i] * d[j] for j in range(k)] for i in range(k)])
    hs = np.array([[h[i, j] * d[i] * d[j] for j in range(k)] for i in range(k)])
    # Cholesky of the unit-diagonal Gram matrix
    low = np.zeros((3, 3))
    low[0, 0] = 1.0
    low[1, 0] = gs[0, 1]
    p1 = 1.0 - low[1, 0] * low[1, 0]
    if not p1 >= PIVOT_MIN:
        return None
    low[1, 1] = math.sqrt(p1)
    if k == 3:
        low[2, 0] = gs[0, 2]
        low[2, 1] = (gs[1, 2] - low[2, 0] * low[1, 0]) / low[1, 1]
        p2 = 1.0 - low[2, 0] * low[2, 0] - low[2, 1] * low[2, 1]
        if not p2 >= PIVOT_MIN:
            return None
        low[2, 2] = math.sqrt(p2)
    # C = L^-1 Hs L^-T
    w = np.zeros((3, 3))
    for j in range(k):
        for i in range(k):
            s = hs[i, j]
            for m in range(i):
                s -= low[i, m] * w[m, j]
            w[i, j] = s / low[i, i]
    c = np.zeros((3, 3))
    for i in range(k):
        for j in range(k):
            s = w[i, j]
            for m in range(j):
                s -= c[i, m] * low[j, m]
            c[i, j] = s / low[j, j]
    for i in range(k):
        for j in range(i + 1, k):
            c[i, j] = c[j, i] = 0.5 * (c[i, j] + c[j, i])
    # cyclic Jacobi
    v = np.eye(3)
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p in range(k - 1):
            for q in range(p + 1, k):
                apq = c[p, q]
                if abs(apq) <= JACOBI_SKIP * (abs(c[p, p]) + abs(c[q, q])):
                    c[p, q] = c[q, p] = 0.0
                    continue
                rotated = True
                tau = (c[q, q] - c[p, p]) / (2.0 * apq)
                t = math.copysign(1.0, tau) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                cs = 1.0 / math.sqrt(1.0 + t * t)
                sn = t * cs
                c[p, p] -= t * apq
                c[q, q] += t * apq
                c[p, q] = c[q, p] = 0.0
                for m in range(k):
                    if m != p and m != q:
                        amp, amq = c[m, p], c[m, q]
                        c[m, p] = c[p, m] = cs * amp - sn * amq
                        c[m, q] = c[q, m] = sn * amp + cs * amq
                for m in range(k):
                    vmp, vmq = v[m, p], v[m, q]
                    v[m, p] = cs * vmp - sn * vmq
                    v[m, q] = sn * vmp + cs * vmq
        if not rotated:
            break
    best = 0
    for i in range(1, k):
        if c[i, i] < c[best, best]:
            best = i
    # coefficients: z = L^-T y, c = D z, scaled to unit G-norm, first coefficient non-negative
    z = np.zeros(3)
    for i in range(k - 1, -1, -1):
        s = v[i, best]
        for m in range(i + 1, k):
            s -= low[m, i] * z[m]
        z[i] = s / low[i, i]
    co = np.array([z[i] * d[i] for i in range(3)])
    nrm2 = 0.0
    for i in range(k):
        for j in range(k):
            nrm2 += co[i] * g[i, j] * co[j]
    if not (nrm2 > 0.0 and math.isfinite(nrm2)):
        return None
    scale = 1.0 / math.sqrt(nrm2)
    if co[0] < 0.0:
        scale = -scale
    co = co * scale
    theta = 0.0
    for i in range(k):
        for j in range(k):
            theta += co[i] * h[i, j] * co[j]
    if not (math.isfinite(theta) and np.isfinite(co).all()):
        return None
    return theta, co


def geneig_lowest(k, G, H):
    """xrs_geneig_lowest restated: (used, theta, c) for the k x k pencil (k = 2, 3) given by its upper triangles;
    used = k, k - 1 after dropping the last basis vector, or 0 on breakdown."""
    g, h = np.zeros((3, 3)), np.zeros((3, 3))
    g[:k, :k], h[:k, :k] = _unpack(k, np.asarray(G, dtype=np.float64)), _unpack(k, np.asarray(H, dtype=np.float64))
    if not (np.isfinite(g).all() and np.isfinite(h).all()):
        return 0, 0.0, np.zeros(3)
    for kk in ((3, 2) if k == 3 else (2,)):
        res = _geneig_try(kk, g, h)
        if res is not None:
            return kk, res[0], res[1]
    return 0, 0.0, np.zeros(3)


# ------------------------------------------------------------------------------------------- the iteration
def lobpcg(matvec, x0, tol, max_iter=0, check_every=1, info=None):
    """xrs_als_local_eig restated: LOBPCG with block size 1 and no preconditioner for the smallest eigenvalue. The
    device state (done, skip, status, iters) is updated every iteration, the host looks at `done` every check_every
    iterations and once after the initialisation, and a frozen iteration changes nothing.
    Returns (x, theta, iters, relres, status); info (a dict) receives the number of steps that dropped p."""
    N = x0.size
    cap = 4 * N + 50
    if max_iter == 0 or max_iter > cap:
        max_iter = cap
    x = np.array(x0, dtype=np.float64)
    dot = lambda a, b: float(np.sum(a * b))  # noqa: E731
    xx = dot(x, x)
    ok = xx > 0.0 and math.isfinite(xx)
    if ok:
        x *= 1.0 / math.sqrt(xx)
    ax = matvec(x)
    theta, nax2 = dot(x, ax), dot(ax, ax)
    r = ax - theta * x
    rr = dot(r, r)
    p, ap = np.zeros_like(x), np.zeros_like(x)
    drops = 0
    relres = lambda: math.sqrt(rr / nax2) if nax2 > 0.0 else 0.0  # noqa: E731
    if not (ok and math.isfinite(theta) and math.isfinite(nax2) and math.isfinite(rr)):
        return x, theta, 0, relres(), BREAKDOWN
    thresh = tol * tol * nax2
    done, status, iters = rr <= thresh, CONVERGED, 0
    seen, k = done, 0
    while k < max_iter and not seen:
        ar = matvec(r)
        # (i) the Gram pair of S = [x, r, p]
        G = [dot(x, x), dot(x, r), dot(x, p), dot(r, r), dot(r, p), dot(p, p)]
        H = [dot(x, ax), dot(x, ar), dot(x, ap), dot(r, ar), dot(r, ap), dot(p, ap)]
        # (ii) the small problem and the fused update
        if done:
            skip = True
        else:
            if iters == 0:
                used, th, c = geneig_lowest(2, [G[0], G[1], G[3]], [H[0], H[1], H[3]])
            else:
                used, th, c = geneig_lowest(3, G, H)
                drops += used == 2
            if used == 0:
                status, skip = BREAKDOWN, True
            else:
                p = c[1] * r + c[2] * p
                ap = c[1] * ar + c[2] * ap
                x = c[0] * x + p
                ax = c[0] * ax + ap
                r = ax - th * x
                theta_next, skip = th, False
        # (iii) the state words
        if skip:
            done = True
        else:
            rr = dot(r, r)
            theta = theta_next
            iters += 1
            if not math.isfinite(rr):
                status, done = BREAKDOWN, True
            elif rr <= thresh:
                done = True
        k += 1
        if k % check_every == 0 or k == max_iter:
            seen = done
    if info is not None:
        info["drops"] = drops
    return x, theta, iters, relres(), (status if done else MAX_ITER)


# ------------------------------------------------------------------------------------------- the sweep
def _move_core(cores, pos, to):
    """One QR (RQ) core move pos -> to = pos +- 1, ranks kept."""
    a = cores[pos]
    rl, n, rr = a.shape
    if to == pos + 1:
        q, rm = np.linalg.qr(a.reshape(rl * n, rr))
        cores[pos] = q.reshape(rl, n, -1)
        cores[to] = np.einsum('ab,bnc->anc', rm, cores[to])
    else:
        q, rm = np.linalg.qr(a.reshape(rl, n * rr).T)
        cores[pos] = q.T.reshape(-1, n, rr)
        cores[to] = np.einsum('anb,bc->anc', cores[to], rm.T)


def sweep(op_cores, x_cores, num_half_sweeps, eps=0.0, tol=1e-10, max_iter=0, history=None):
    """ALS_EIGEN restated: core to site 0, x normalised, then half sweeps of local eigenproblems (lobpcg from the
    current core) with ALS's end rule on lambda. Requires ranks that QR keeps (r_k <= r_{k-1} n_k and the mirror
    image). Returns (lambda, cores) with the core where the last half sweep ended."""
    cores = [np.array(c, dtype=np.float64) for c in x_cores]
    d = len(cores)
    for k in range(d - 1, 0, -1):
        _move_core(cores, k, k - 1)
    cores[0] /= np.linalg.norm(cores[0])
    pos, step, count = 0, 1, 0
    last2, last, lam = 1e102, 1e101, 1e100
    while True:
        L, R = lr.environments(op_cores, cores, pos, False)
        A = op_cores[pos]
        x, theta, iters, relres, status = lobpcg(lambda v: lr.apply_chain(v, L, A, R, False), cores[pos], tol, max_iter, 16)
        if status == BREAKDOWN:
            raise RuntimeError("local eigenproblem at site %d broke down" % pos)
        cores[pos] = x
        if d == 1 or (step == 1 and pos == d - 1) or (step == -1 and pos == 0):
            count += 1
            last2, last, lam = last, lam, theta
            if history is not None:
                history.append(lam)
            if d == 1 or count == num_half_sweeps or abs(last - lam) < eps or abs(last2 - lam) < eps:
                return lam, cores
            step = -step
        _move_core(cores, pos, pos + step)
        pos += step


# ------------------------------------------------------------------------------------------- test problems
EXTRA_SHAPES = [(1, 1, 1, 1, 1), (1, 2, 1, 1, 1), (1, 3, 1, 2, 1), (2, 2, 1, 1, 2)]
SHAPES = lr.SHAPES + EXTRA_SHAPES


def check_eigenpair(p, x, theta, iters, relres, status, tol):
    """The bars of the iteration tests, CPU and GPU: status 0, returned relres <= tol, true residual
    <= 2 tol, unit norm to 1e-13, theta against eigvalsh to 1e-12 w_max (the worst-case N eps bound of an N = 4092
    dot product; the Rayleigh quotient's own error ||r||^2 / gap is below rounding), and Davis-Kahan for the angle."""
    N = p.N
    w, V = np.linalg.eigh(0.5 * (p.M + p.M.T))
    wmax = np.abs(w).max()
    x0 = p.x0.reshape(N) / np.linalg.norm(p.x0)
    nax0 = np.linalg.norm(p.M @ x0)
    xv = x.reshape(N)
    res = np.linalg.norm(p.M @ xv - theta * xv)
    true_res = res / nax0
    sin = np.linalg.norm(xv - V[:, 0] * (V[:, 0] @ xv)) / np.linalg.norm(xv)
    print("dims %s: iters %d relres %.3e true residual %.3e | ||x|| - 1 | %.1e theta error %.2e w_max sin %.2e" %
          (p.dims, iters, relres, true_res, abs(np.linalg.norm(xv) - 1.0), abs(theta - w[0]) / wmax, sin))
    assert status == CONVERGED
    assert 0 <= iters <= 4 * N + 50
    assert relres <= tol, relres
    assert true_res <= 2 * tol, true_res
    assert abs(np.linalg.norm(xv) - 1.0) <= 1e-13
    assert abs(theta - w[0]) <= 1e-12 * wmax, (theta, w[0])
    if N > 1:
        assert sin <= 2 * res / (w[1] - w[0]), (sin, res, w[1] - w[0])


def laplace_cores(d, n, shift=0.0):
    return [lr.laplace_core(n, 1 if k == 0 else 2, 1 if k == d - 1 else 2, shift) for k in range(d)]


def perturbed_cores(d, n):
    """The Laplace cores plus 0.15 (E + E^T over the two middle modes), E standard normal from default_rng(11)."""
    rng = np.random.default_rng(11)
    out = []
    for c in laplace_cores(d, n):
        e = rng.standard_normal(c.shape)
        out.append(c + 0.15 * (e + e.transpose(0, 2, 1, 3)))
    return out


def laplace_lowest(d, n):
    """(lambda_1, lambda_2, the unit rank-one sine eigenvector as a dense tensor) of the d-dimensional Laplacian."""
    mu = 2.0 - 2.0 * np.cos(np.pi * np.arange(1, 3) / (n + 1))
    s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
    s /= np.linalg.norm(s)
    v = s
    for _ in range(d - 1):
        v = np.multiply.outer(v, s)
    return d * mu[0], (d - 1) * mu[0] + mu[1], v


def op_dense(op_cores):
    """The operator as a matrix (row modes first)."""
    d = len(op_cores)
    t = op_cores[0]
    for c in op_cores[1:]:
        t = np.tensordot(t, c, axes=([-1], [0]))
    t = t.reshape(t.shape[1:-1])                       # (i1, j1, i2, j2, ...)
    t = t.transpose(list(range(0, 2 * d, 2)) + list(range(1, 2 * d, 2)))
    N = int(np.prod(t.shape[:d]))
    return t.reshape(N, N)


def tt_dense(cores):
    t = cores[0]
    for c in cores[1:]:
        t = np.tensordot(t, c, axes=([-1], [0]))
    return t.reshape(t.shape[1:-1])


def random_start(dims, ranks, seed):
    rng = np.random.default_rng(seed)
    r = [1] + list(ranks) + [1]
    return [rng.standard_normal((r[k], dims[k], r[k + 1])) for k in range(len(dims))]
