"""The certified truncating round's eigensolver (xrs_sym_eig_top, csrc/syev.hip) vs LAPACK dsyevd (numpy):
the kk largest eigenpairs of symmetric matrices up to 256, with flat, graded and clustered-free spectra.
Bars: eigenvalues to 1e-13 ||A||, eigenvectors orthonormal to 1e-12 and residual ||A u - lam u|| to 1e-12 ||A||
(the round additionally checks the orthonormality of every new core and falls back on failure).
test_sym_eig_top_spectra runs the same bars over the matrix classes of tests/syev_spectra.py: clusters of 16 to 64
(nearly) equal eigenvalues at the top of, inside and across the kept set, scalar and rank-deficient matrices,
tridiagonals that split, indefinite and negative definite matrices, Wilkinson matrices, order 2 and the orders
at which the kernels switch (tests/test_syev_spectra_cpu.py shows that LAPACK itself meets the bars on each).
The contract (xerus_amd.h): a cluster of any size comes back orthonormal with status 0, which is what every case
here asserts; a solver that cannot deliver that reports a negative status, never a wrong vector with status 0."""
import numpy as np
import pytest

import syev_spectra as sp

pytestmark = pytest.mark.gpu


def _spd(n, spectrum, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * spectrum) @ Q.T


@pytest.mark.parametrize("n,kk,kind", [(2, 1, "flat"), (5, 5, "flat"), (33, 7, "flat"), (64, 64, "flat"), (64, 32, "graded"),
                                       (100, 50, "flat"), (128, 64, "flat"), (128, 48, "graded"), (128, 20, "wishart"),
                                       (129, 60, "flat"), (200, 100, "wishart"), (256, 128, "wishart"), (256, 256, "flat")])
def test_sym_eig_top(handle, n, kk, kind):
    rng = np.random.default_rng(n * 7 + kk)
    if kind == "flat":
        A = _spd(n, 1.0 + rng.random(n) * 3.0, n)
    elif kind == "graded":   # gaps >= 7e-4 ||A|| among the kept ones (inverse iteration: orthogonality ~ u ||A|| / gap)
        A = _spd(n, 0.9 ** np.arange(n), n + 1)
    else:   # the round's P = B B^T of a random wide edge
        B = rng.standard_normal((n, 20 * n))
        A = B @ B.T
    A = 0.5 * (A + A.T)
    lam, Ut, st = handle.sym_eig_top(handle.array(A), kk)
    assert st == 0
    lam, U = lam.numpy(), Ut.numpy().T
    want = np.linalg.eigvalsh(A)[::-1][:kk]
    nrm = np.linalg.norm(A, 2)
    assert np.abs(lam - want).max() <= 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(kk)).max() <= 1e-12
    assert np.linalg.norm(A @ U - U * lam, axis=0).max() <= 1e-12 * nrm


def test_sym_eig_top_lower_triangle_only(handle):
    """Only the lower triangle is read (the round's Grams are mirrored anyway)."""
    A = _spd(40, np.linspace(1, 5, 40), 3)
    Al = np.tril(A) + np.triu(np.full_like(A, 7.0), 1)
    lam, Ut, st = handle.sym_eig_top(handle.array(Al), 10)
    assert st == 0
    assert np.abs(lam.numpy() - np.linalg.eigvalsh(A)[::-1][:10]).max() <= 1e-13 * 5


@pytest.mark.parametrize("n,kk", [(24, 12), (96, 40), (200, 120)])
def test_sym_eig_top_clusters(handle, n, kk):
    """Exactly repeated and 1e-9-close eigenvalues inside the kept set (inverse iteration alone gives
    non-orthogonal vectors there; k_cluster_orth orthonormalises each cluster): eigenvalues, orthonormality
    and residuals at the same bars, and the kept subspace equals LAPACK's when the cut lies in a gap."""
    rng = np.random.default_rng(n)
    spec = np.concatenate([np.repeat([9.0, 7.0, 5.0], 4), 5.0 - 1e-9 * np.arange(1, 4), 1.0 + rng.random(n - 15)])
    A = _spd(n, spec, n + 3)
    A = 0.5 * (A + A.T)
    lam, Ut, st = handle.sym_eig_top(handle.array(A), kk)
    assert st == 0
    lam, U = lam.numpy(), Ut.numpy().T
    w, Z = np.linalg.eigh(A)
    nrm = np.linalg.norm(A, 2)
    assert np.abs(lam - w[::-1][:kk]).max() <= 1e-13 * nrm
    assert np.abs(U.T @ U - np.eye(kk)).max() <= 1e-12
    assert np.linalg.norm(A @ U - U * lam, axis=0).max() <= 1e-12 * nrm
    P = Z[:, ::-1][:, :kk]
    if w[::-1][kk - 1] - w[::-1][kk] > 1e-3:   # the projector onto the kept subspace is unique
        assert np.abs(U @ U.T - P @ P.T).max() <= 1e-11


@pytest.fixture(scope="module")
def lapack():
    """(A, meta, eigenvalues descending, eigenvectors) of a generator of syev_spectra, computed once."""
    cache = {}

    def get(cid, gen):
        key = cid.rsplit("-kk", 1)[0]
        if key not in cache:
            A, meta = gen()
            w, Z = np.linalg.eigh(A)
            for x in (A, w, Z):
                x.setflags(write=False)
            cache[key] = (A, meta, w[::-1], Z[:, ::-1])
        return cache[key]
    return get


@pytest.mark.parametrize("cid,family,gen,kk", sp.CASES, ids=sp.IDS)
def test_sym_eig_top_spectra(handle, lapack, cid, family, gen, kk):
    A, meta, w, Z = lapack(cid, gen)
    lam, Ut, st = handle.sym_eig_top(handle.array(A), kk)
    lam, U = lam.numpy(), Ut.numpy().T
    nrm = np.linalg.norm(A, 2)
    e_lam = np.abs(lam - w[:kk]).max() / nrm
    e_orth = np.abs(U.T @ U - np.eye(kk)).max()
    e_res = np.linalg.norm(A @ U - U * lam, axis=0).max() / nrm
    unique = sp.projector_unique(meta, kk)
    e_proj = np.abs(U @ U.T - Z[:, :kk] @ Z[:, :kk].T).max() if unique else float("nan")
    print(f"sym_eig_top {cid}: status {st} eigenvalues {e_lam:.2e} orthogonality {e_orth:.2e} residual {e_res:.2e} projector {e_proj:.2e}")
    assert st == 0
    assert e_lam <= 1e-13
    assert e_orth <= 1e-12
    assert e_res <= 1e-12
    if unique:
        assert e_proj <= 1e-11


@pytest.mark.parametrize("cid", ["a-m25-middle-exact-kk35", "c-gram200x50-kk200"])
def test_sym_eig_top_is_bit_deterministic(handle, lapack, cid):
    """The sharded round runs an edge replicated on every rank and relies on identical results."""
    _, _, gen, kk = sp.CASES[sp.IDS.index(cid)]
    A = lapack(cid, gen)[0]
    lam1, Ut1, st1 = handle.sym_eig_top(handle.array(A), kk)
    lam2, Ut2, st2 = handle.sym_eig_top(handle.array(A), kk)
    assert st1 == 0 and st2 == 0
    assert np.array_equal(lam1.numpy(), lam2.numpy())
    assert np.array_equal(Ut1.numpy(), Ut2.numpy())
