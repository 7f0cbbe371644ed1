"""Symmetric test matrices for the eigensolver suite (tests/test_syev_gpu.py, tests/test_syev_spectra_cpu.py):
pure-numpy generators returning (A, meta). A is exactly symmetric; meta carries
  spec      the intended spectrum, descending (of a structured matrix: LAPACK's, descending),
  clusters  [(first, members)]: the groups of (nearly) equal eigenvalues as index ranges into spec,
  tol       how far apart (relative to ||A||) the members of a cluster may lie.
Random matrices are Q diag(spec) Q^T with a seeded Haar Q; where the structure is the point (a Gram of a thin
factor, a block-diagonal, a diagonal, Toeplitz, Wilkinson, G + G^T) the matrix is built as such.
CASES lists every (id, family, generator, kk) the GPU suite runs."""
import numpy as np


def haar(n, seed):
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def _sym(A):
    return 0.5 * (A + A.T)


def _meta(spec, clusters=(), tol=0.0):
    return {"spec": np.sort(np.asarray(spec, dtype=float))[::-1], "clusters": list(clusters), "tol": tol}


def from_spectrum(spec, seed, clusters=(), tol=0.0):
    spec = np.asarray(spec, dtype=float)
    Q = haar(len(spec), seed)
    return _sym((Q * spec) @ Q.T), _meta(spec, clusters, tol)


def _from_lapack(A, clusters=(), tol=0.0):
    A = _sym(A)
    return A, _meta(np.linalg.eigvalsh(A), clusters, tol)


def cluster_spectrum(n, mult, above, spread, step):
    """||A|| = 10: `above` distinct values from 10 downwards in steps of `step`, a gap of 0.5, `mult` members
    `spread` * ||A|| apart, a gap of 0.5, the remaining values in steps of `step`."""
    top = 10.0 - step * np.arange(above)
    c = top[-1] - 0.5 if above else 10.0
    cl = c - 10.0 * spread * np.arange(mult)
    rest = cl[-1] - 0.5 - step * np.arange(n - mult - above)
    spec = np.concatenate([top, cl, rest])
    assert spec[-1] > 0.1 and np.all(np.diff(spec) <= 0.0)
    return spec


def cluster(n, mult, layout, spread, seed, kk, step=0.1025, above=None):
    """One cluster of `mult` members in a spectrum of distinct values with gaps > 1e-2 ||A|| (step 0.1025, ||A|| = 10).
    layout: "top" (the cluster leads), "middle" (5 distinct above it, the cut below it in the distinct tail),
    "straddle" (the cut kk falls into the cluster's middle); `above` overrides the number of distinct values above it."""
    if above is None:
        above = {"top": 0, "middle": 5, "straddle": kk - mult // 2}[layout]
    spec = cluster_spectrum(n, mult, above, spread, step)
    return from_spectrum(spec, seed, [(above, mult)], 2.0 * spread * mult)


def scalar(n, c=2.5):
    return c * np.eye(n), _meta(np.full(n, c), [(0, n)])


def near_scalar(n, seed, eps=1e-10):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return _from_lapack(np.eye(n) + eps * _sym(G), [(0, n)], 4.0 * eps * np.sqrt(n))


def gram(n, r, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, r))
    s = np.linalg.svd(B, compute_uv=False)
    return _sym(B @ B.T), _meta(np.concatenate([s * s, np.zeros(n - r)]), [(r, n - r)], 1e-13)


def twin_blocks(m, seed):
    """diag(A1, A1), A1 = Q diag(linspace(1, 4, m)) Q^T: every eigenvalue exactly double, its two vectors in
    different blocks; the tridiagonal splits in the middle."""
    s1 = np.linspace(4.0, 1.0, m)
    A1, _ = from_spectrum(s1, seed)
    A = np.zeros((2 * m, 2 * m))
    A[:m, :m] = A1
    A[m:, m:] = A1
    return A, _meta(np.repeat(s1, 2), [(2 * i, 2) for i in range(m)])


def diagonal(values, seed):
    values = np.asarray(values, dtype=float)
    d = np.random.default_rng(seed).permutation(values)
    s = np.sort(values)[::-1]
    first = [i for i in range(len(s)) if i == 0 or s[i] != s[i - 1]]
    sizes = np.diff(first + [len(s)])
    return np.diag(d), _meta(s, [(f, int(c)) for f, c in zip(first, sizes) if c > 1])


def toeplitz(n):
    A = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    return A, _meta(2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))


def indefinite(n, seed):
    G = np.random.default_rng(seed).standard_normal((n, n))
    return _from_lapack(G + G.T)


def negative_definite(n, seed):
    rng = np.random.default_rng(seed)
    return from_spectrum(-(1.0 + 3.0 * rng.random(n)), seed + 1)


def flat_spd(n, seed):
    rng = np.random.default_rng(seed)
    return from_spectrum(1.0 + 3.0 * rng.random(n), seed + 1)


def wilkinson(m):
    """W+_{2m+1}: diagonal |m|, ..., 1, 0, 1, ..., |m|, off-diagonals 1."""
    n = 2 * m + 1
    return np.diag(np.abs(np.arange(n) - m).astype(float)) + np.eye(n, k=1) + np.eye(n, k=-1)


def wilkinson_case(m, pairs):
    """The `pairs` largest eigenvalues pairwise agree to ~1e-14 ||A|| and closer."""
    return _from_lapack(wilkinson(m), [(2 * i, 2) for i in range(pairs)], 1e-13)


def glued_wilkinson(m, copies, glue):
    W = wilkinson(m)
    n = W.shape[0]
    A = np.kron(np.eye(copies), W)
    for c in range(1, copies):
        A[c * n - 1, c * n] = A[c * n, c * n - 1] = glue
    # (the top eigenvalue of each copy is a close pair; the glue couples the copies at O(glue))
    return _from_lapack(A, [(0, 2 * copies)], 4.0 * glue / m)


def order2(a, b):
    return np.array([[a, b], [b, a]]), _meta([a + abs(b), a - abs(b)], [(0, 2)] if abs(b) < 1e-3 * abs(a) else [], 4.0 * abs(b) / abs(a))


def signed_identity2():
    return np.array([[1.0, 0.0], [0.0, -1.0]]), _meta([1.0, -1.0])


def _cases():
    cs = []

    def add(family, name, gen, kk):
        cs.append((f"{family}-{name}-kk{kk}", family, gen, kk))

    # (a) one large cluster at order 96, exact and 1e-12 ||A|| apart; one case at order 256
    for mult in (16, 17, 18, 20, 24, 25, 34, 40):
        for layout in ("top", "middle", "straddle"):
            for sname, spread in (("exact", 0.0), ("near", 1e-12)):
                kk = mult + 10
                add("a", f"m{mult}-{layout}-{sname}",
                    lambda mult=mult, layout=layout, spread=spread, kk=kk: cluster(96, mult, layout, spread, 1000 + mult, kk), kk)
    # (order 256: 32 distinct values above the cluster and 32 below it inside the kept 128, gaps 4.5e-3 ||A||)
    add("a", "n256-m64-middle-exact", lambda: cluster(256, 64, "middle", 0.0, 2064, 128, step=0.045, above=32), 128)
    # (b) scalar and near-scalar
    for n in (2, 20, 64, 65, 256):
        for kk in (1, n):
            add("b", f"scalar{n}", lambda n=n: scalar(n), kk)
    add("b", "near-scalar128", lambda: near_scalar(128, 7), 64)
    # (c) rank-deficient Grams
    for n, r in ((64, 10), (200, 50)):
        for kk in (r, r + 1, n):
            add("c", f"gram{n}x{r}", lambda n=n, r=r: gram(n, r, n + r), kk)
    # (d) split tridiagonals
    for kk in (20, 80):
        add("d", "twins40", lambda: twin_blocks(40, 11), kk)
    for n in (80, 200):
        for kk in (n // 2, n):
            add("d", f"diagperm{n}", lambda n=n: diagonal(np.arange(1, n + 1), n), kk)
    for kk in (40, 42, 80):
        add("d", "diagrep80", lambda: diagonal(np.repeat(np.arange(1, 21), 4), 5), kk)
    for kk in (1, 64, 129):
        add("d", "toeplitz129", lambda: toeplitz(129), kk)
    # (e) signs
    for n in (33, 129):
        for kk in (1, n // 2, n):
            add("e", f"indefinite{n}", lambda n=n: indefinite(n, 3 * n), kk)
            add("e", f"negdef{n}", lambda n=n: negative_definite(n, 5 * n), kk)
    # (f) Wilkinson
    for m, pairs in ((10, 1), (50, 20)):
        for kk in (10, 2 * m + 1):
            add("f", f"wilkinson{2 * m + 1}", lambda m=m, pairs=pairs: wilkinson_case(m, pairs), kk)
    for kk in (6, 12, 63):
        add("f", "glued21x3", lambda: glued_wilkinson(10, 3, 1e-8), kk)
    # (g) order 2
    for b in (0.0, 1e-300, 1e-8, 1.0):
        for kk in (1, 2):
            add("g", f"ab-{b:g}", lambda b=b: order2(1.5, b), kk)
    for kk in (1, 2):
        add("g", "pm1", signed_identity2, kk)
    # (h) the orders at which the tridiagonalisation and back-transformation kernels switch
    for n in (64, 65, 128, 129, 256):
        for kk in (1, n):
            add("h", f"flat{n}", lambda n=n: flat_spd(n, 7 * n), kk)
    return cs


CASES = _cases()
IDS = [c[0] for c in CASES]


def projector_unique(meta, kk):
    """The projector onto the kk leading eigenvectors is compared only where the cut lies in a gap > 1e-3 ||A||."""
    s = meta["spec"]
    return kk < len(s) and s[kk - 1] - s[kk] > 1e-3 * np.abs(s).max()
